// records_kernels.hip -- librpcc_records.so: NCLT velodyne_sync records -> stored rows (include/rpcc_records.h) for gfx950.
//
// One elementwise launch, bound by memory: 8 bytes read and 16 written per point.  A lane takes TWO records with one 16-byte load (the
// widest global access; 8-byte accesses run at 0.54-0.70 of its rate) and writes their two rows with two 16-byte stores, 32 contiguous
// bytes per lane.  The 16-byte loads need a 16-byte aligned address and records are only 8-byte aligned, so the pairs start at the first
// 16-byte boundary: `head` (0 or 1) records stand in front of it and (total - head) & 1 behind the last pair; one lane of the first
// workgroup unpacks those with 8-byte loads.  The grid is capped at REC_GRID_CAP workgroups and strides over the pairs.  No LDS, no
// atomics; every row is written by exactly one lane.  The rule itself is records_rule.h.
#include <algorithm>

#include "../../include/rpcc_records.h"
#include "../csrc_tile/tiles.h"
#include "records_rule.h"

static_assert(RPCC_RECORDS_ERR_ARG == TILE_ERR_ARG && RPCC_RECORDS_ERR_HIP == TILE_ERR_HIP, "rpcc_records.h and tiles.h disagree");
static_assert(RPCC_RECORDS_BYTES == RECORDS_BYTES && sizeof(uint2) == RECORDS_BYTES, "a record is two 32-bit words");

#define REC_THREADS 256     // lanes of a workgroup, one pair of records per lane and trip
#define REC_GRID_CAP 2048   // workgroups at most (256 CUs x 8): the loop strides over the rest

extern "C" int rpcc_records_version(void) { return RPCC_RECORDS_ABI_VERSION; }
extern "C" const char *rpcc_records_last_error(void) { return g_err; }

__device__ __forceinline__ float4 unpack_row(uint32_t w0, uint32_t w1) {
    float r[4];
    records_row(w0, w1, r);
    return make_float4(r[0], r[1], r[2], r[3]);
}

// rec: the records, 8-byte aligned; rec + head is 16-byte aligned.  npairs = (total - head) / 2.
__global__ __launch_bounds__(REC_THREADS) void records_unpack_kernel(const uint2 *__restrict__ rec, int64_t total, int head, int64_t npairs,
                                                                     float4 *__restrict__ rows) {
    const uint4 *__restrict__ pairs = (const uint4 *)(rec + head);
    for (int64_t p = (int64_t)blockIdx.x * REC_THREADS + threadIdx.x; p < npairs; p += (int64_t)gridDim.x * REC_THREADS) {
        const uint4 v = pairs[p];
        const int64_t r = head + 2 * p;
        rows[r] = unpack_row(v.x, v.y);
        rows[r + 1] = unpack_row(v.z, v.w);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {   // the records the pairs leave out: one in front, one behind, or neither
        if (head) {
            const uint2 v = rec[0];
            rows[0] = unpack_row(v.x, v.y);
        }
        if (head + 2 * npairs < total) {
            const uint2 v = rec[total - 1];
            rows[total - 1] = unpack_row(v.x, v.y);
        }
    }
}

extern "C" int rpcc_records_unpack(const void *records, int64_t total, float *rows, void *stream) {
    ARG_TRY(total >= 0 && total <= RPCC_RECORDS_MAX_TOTAL);
    ARG_TRY((uintptr_t)records % RPCC_RECORDS_BYTES == 0 && (uintptr_t)rows % 16 == 0);
    if (total == 0) return 0;
    ARG_TRY(records && rows);
    const uintptr_t r0 = (uintptr_t)records, r1 = r0 + (uintptr_t)total * RPCC_RECORDS_BYTES, o0 = (uintptr_t)rows, o1 = o0 + (uintptr_t)total * 16;
    ARG_TRY(r1 <= o0 || o1 <= r0);   // no overlap: a row would be written over records not yet read
    const int head = (int)((r0 % 16) / RPCC_RECORDS_BYTES);      // records in front of the first 16-byte boundary (total >= 1 >= head)
    const int64_t npairs = (total - head) / 2;
    const unsigned wgs = (unsigned)std::max<int64_t>(std::min<int64_t>((npairs + REC_THREADS - 1) / REC_THREADS, REC_GRID_CAP), 1);
    records_unpack_kernel<<<wgs, REC_THREADS, 0, (hipStream_t)stream>>>((const uint2 *)records, total, head, npairs, (float4 *)rows);
    LAUNCH_CHECK();
    return 0;
}
