// fields_kernels.hip -- librpcc_fields.so: the point records of .pcd / .ply files -> stored rows (include/rpcc_fields.h) for gfx950.
//
// One launch for the B frames of a chunk, bound by memory.  Records are not naturally aligned (a 22-byte stride behind a header of odd
// length: a float straddles two dwords), so no lane loads a field from global memory.  A workgroup takes a TILE of a frame --
// fields_tile_rows(step) points, FIELDS_STAGE_BYTES of records at most --, brings the tile's contiguous byte range into LDS with
// aligned 16-byte loads, several per lane in flight (the chunk's base is 16-byte aligned; the range is widened to 16-byte boundaries and
// a last part chunk at the very end of `bytes` is read byte by byte, so no address outside bytes .. bytes + nbytes is touched), and the
// lanes take the tile's points in turn: a point's four elements are assembled from LDS dwords and written as ONE 16-byte row.  Where the
// four columns' ranges do not fit one stage together (planes: a decompressed binary_compressed body of more than a thousand points) the
// columns are staged one after the other through the same LDS and every column is written with 4-byte stores, a NONE column as +0.0.
//
// The grid is (FX, FY): workgroup (x, y) takes the frames y, y + FY, ... and of each the tiles x, x + FX, ...; FX * FY <= FLD_GRID_CAP.
// The descriptor is validated (fields_rule.h) by every workgroup before it reads a byte of the frame; workgroup x == 0 writes the
// status.  No atomics; every row is written by exactly one lane.
#include <algorithm>

#include "../../include/rpcc_fields.h"
#include "../csrc_tile/tiles.h"
#include "fields_rule.h"

static_assert(RPCC_FIELDS_ERR_ARG == TILE_ERR_ARG && RPCC_FIELDS_ERR_HIP == TILE_ERR_HIP, "rpcc_fields.h and tiles.h disagree");
static_assert(RPCC_FIELDS_DESC_WORDS == FIELDS_DESC_WORDS && RPCC_FIELDS_MAX_STEP == FIELDS_MAX_STEP, "rpcc_fields.h and fields_rule.h disagree");
static_assert(RPCC_FIELDS_T_NONE == FIELDS_T_NONE && RPCC_FIELDS_T_F32 == FIELDS_T_F32 && RPCC_FIELDS_T_F64 == FIELDS_T_F64 &&
              RPCC_FIELDS_T_I8 == FIELDS_T_I8 && RPCC_FIELDS_T_U8 == FIELDS_T_U8 && RPCC_FIELDS_T_I16 == FIELDS_T_I16 &&
              RPCC_FIELDS_T_U16 == FIELDS_T_U16 && RPCC_FIELDS_T_I32 == FIELDS_T_I32 && RPCC_FIELDS_T_U32 == FIELDS_T_U32 &&
              RPCC_FIELDS_E_LAYOUT == FIELDS_E_LAYOUT, "rpcc_fields.h and fields_rule.h disagree");

#define FLD_THREADS 256     // lanes of a workgroup; they take a tile's points in turn
#define FLD_GRID_CAP 2048   // workgroups at most (256 CUs x 8): the loops stride over the rest
// LDS of a stage in 16-byte chunks: FIELDS_STAGE_BYTES, up to 15 bytes in front of the range and behind it (the 16-byte boundaries), and
// the dwords an element's assembly reads past its last byte
#define FLD_LDS_CHUNKS (FIELDS_STAGE_BYTES / 16 + 4)
static_assert(FIELDS_TILE_MAX_ROWS % FLD_THREADS == 0, "a full tile gives every lane the same number of points");
static_assert(FLD_LDS_CHUNKS * 16 >= FIELDS_STAGE_BYTES + 16 + 12 + 16, "stage: range + front slack + over-read + rounding");

extern "C" int rpcc_fields_version(void) { return RPCC_FIELDS_ABI_VERSION; }
extern "C" const char *rpcc_fields_last_error(void) { return g_err; }

// Bytes [lo, hi) of the chunk -> LDS, from the 16-byte boundary a0 = lo & ~15 on.  0 <= lo < hi <= nbytes, hi - a0 <= STAGE + 16.
__device__ __forceinline__ void stage(const uint8_t *__restrict__ bytes, int64_t nbytes, int64_t a0, int64_t hi, uint4 *s_stage) {
    const int nchunks = (int)((hi - a0 + 15) >> 4);
    for (int k = threadIdx.x; k < nchunks; k += FLD_THREADS) {
        const int64_t o = a0 + 16 * (int64_t)k;
        uint4 v;
        if (o + 16 <= nbytes) {
            v = *(const uint4 *)(bytes + o);
        } else {   // the part chunk at the very end of the buffer (one per call at most)
            uint32_t w[4] = {0u, 0u, 0u, 0u};
            for (int j = 0; o + j < nbytes; ++j) w[j >> 2] |= (uint32_t)bytes[o + j] << (8 * (j & 3));
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
        s_stage[k] = v;
    }
}

// The fp32 bits of the element of `type` whose first byte is byte p of the stage.
__device__ __forceinline__ uint32_t element(const uint4 *s_stage, int p, int type) {
    const uint32_t *s = (const uint32_t *)s_stage;
    const int q = p >> 2, sh = 8 * (p & 3);
    const uint32_t w0 = s[q], w1 = s[q + 1];
    const uint32_t lo = (uint32_t)(((uint64_t)w1 << 32 | w0) >> sh);
    uint32_t hi = 0u;
    if (type == FIELDS_T_F64) {
        const uint32_t w2 = s[q + 2];
        hi = (uint32_t)(((uint64_t)w2 << 32 | w1) >> sh);
    }
    return fields_bits(type, lo, hi);
}

__global__ __launch_bounds__(FLD_THREADS) void fields_unpack_kernel(const uint8_t *__restrict__ bytes, int64_t nbytes, const int64_t *__restrict__ desc,
                                                                    int B, const int64_t *__restrict__ row_offsets, int64_t total,
                                                                    uint4 *__restrict__ rows, int32_t *__restrict__ status) {
    __shared__ uint4 s_stage[FLD_LDS_CHUNKS];
    const int lane = threadIdx.x;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        int64_t d[FIELDS_DESC_WORDS];
        for (int k = 0; k < FIELDS_DESC_WORDS; ++k) d[k] = desc[(int64_t)b * FIELDS_DESC_WORDS + k];
        const int64_t r0 = row_offsets[b], r1 = row_offsets[b + 1];
        const bool rows_ok = r0 >= 0 && r1 >= r0 && r1 <= total;
        const int st = rows_ok ? fields_validate(d, nbytes, r1 - r0) : FIELDS_E_LAYOUT;
        if (blockIdx.x == 0 && lane == 0) status[b] = st;
        if (!rows_ok) continue;
        if (st != FIELDS_OK) {   // +0.0 rows; nothing of the descriptor is used
            for (int64_t i = (int64_t)blockIdx.x * FLD_THREADS + lane; i < r1 - r0; i += (int64_t)gridDim.x * FLD_THREADS)
                rows[r0 + i] = make_uint4(0u, 0u, 0u, 0u);
            continue;
        }
        const int64_t n = d[FIELDS_D_N], span_off = d[FIELDS_D_SPAN_OFF];
        const int tile_rows = fields_tile_rows(fields_max_step(d));
        const int64_t ntiles = (n + tile_rows - 1) / tile_rows;
        for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
            const int64_t i0 = t * tile_rows;
            const int cnt = (int)std::min<int64_t>(tile_rows, n - i0);
            int64_t lo[4], hi[4], ulo = INT64_MAX, uhi = 0;   // the columns' byte ranges inside the chunk, and their union
            for (int c = 0; c < 4; ++c) {
                if (d[FIELDS_D_TYPE + c] == FIELDS_T_NONE) continue;
                lo[c] = span_off + d[FIELDS_D_OFF + c] + i0 * d[FIELDS_D_STEP + c];
                hi[c] = lo[c] + (cnt - 1) * d[FIELDS_D_STEP + c] + fields_size(d[FIELDS_D_TYPE + c]);
                ulo = std::min(ulo, lo[c]);
                uhi = std::max(uhi, hi[c]);
            }
            if (uhi - (ulo & ~(int64_t)15) <= FIELDS_STAGE_BYTES + 16) {   // records: the four columns share one stage
                const int64_t a0 = ulo & ~(int64_t)15;
                stage(bytes, nbytes, a0, uhi, s_stage);
                __syncthreads();
                for (int r = lane; r < cnt; r += FLD_THREADS) {
                    uint32_t v[4] = {0u, 0u, 0u, 0u};
                    for (int c = 0; c < 4; ++c)
                        if (d[FIELDS_D_TYPE + c] != FIELDS_T_NONE)
                            v[c] = element(s_stage, (int)(lo[c] - a0) + r * (int)d[FIELDS_D_STEP + c], (int)d[FIELDS_D_TYPE + c]);
                    rows[r0 + i0 + r] = make_uint4(v[0], v[1], v[2], v[3]);
                }
                __syncthreads();
            } else {                                                       // planes: one column after the other, 4-byte stores
                uint32_t *words = (uint32_t *)(rows + r0 + i0);
                for (int c = 0; c < 4; ++c) {
                    if (d[FIELDS_D_TYPE + c] == FIELDS_T_NONE) {
                        for (int r = lane; r < cnt; r += FLD_THREADS) words[4 * r + c] = 0u;
                        continue;
                    }
                    const int64_t a0 = lo[c] & ~(int64_t)15;
                    stage(bytes, nbytes, a0, hi[c], s_stage);
                    __syncthreads();
                    for (int r = lane; r < cnt; r += FLD_THREADS)
                        words[4 * r + c] = element(s_stage, (int)(lo[c] - a0) + r * (int)d[FIELDS_D_STEP + c], (int)d[FIELDS_D_TYPE + c]);
                    __syncthreads();
                }
            }
        }
    }
}

extern "C" int rpcc_fields_unpack(const void *bytes, int64_t nbytes, const int64_t *desc, int B, const int64_t *row_offsets, int64_t total,
                                  float *rows, int32_t *status, void *stream) {
    ARG_TRY(B >= 0 && B <= RPCC_FIELDS_MAX_BATCH);
    ARG_TRY(total >= 0 && total <= RPCC_FIELDS_MAX_TOTAL);
    ARG_TRY(nbytes >= 0);
    ARG_TRY((uintptr_t)bytes % 16 == 0 && (uintptr_t)rows % 16 == 0);
    ARG_TRY((uintptr_t)desc % 8 == 0 && (uintptr_t)row_offsets % 8 == 0 && (uintptr_t)status % 4 == 0);
    if (B == 0) {
        ARG_TRY(total == 0);
        return 0;
    }
    ARG_TRY(desc && row_offsets && status);
    ARG_TRY(bytes || nbytes == 0);
    ARG_TRY(rows || total == 0);
    const uintptr_t s0 = (uintptr_t)bytes, s1 = s0 + (uintptr_t)nbytes, o0 = (uintptr_t)rows, o1 = o0 + (uintptr_t)total * 16;
    ARG_TRY(s1 <= o0 || o1 <= s0 || nbytes == 0 || total == 0);   // no overlap: a row would be written over records not yet read
    const int64_t fy = std::min<int64_t>(B, FLD_GRID_CAP);
    const int64_t per_frame = (total / B + FIELDS_TILE_MAX_ROWS - 1) / FIELDS_TILE_MAX_ROWS;   // tiles of an average frame at a full tile's rows
    const int64_t fx = std::max<int64_t>(std::min<int64_t>(per_frame, FLD_GRID_CAP / fy), 1);
    fields_unpack_kernel<<<dim3((unsigned)fx, (unsigned)fy), FLD_THREADS, 0, (hipStream_t)stream>>>(
        (const uint8_t *)bytes, nbytes, desc, B, row_offsets, total, (uint4 *)rows, status);
    LAUNCH_CHECK();
    return 0;
}
