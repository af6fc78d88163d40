// bzip2_kernels.hip -- librpcc_bzip2.so (include/rpcc_bzip2.h): bzip2 streams encoded on gfx950, one 1024-thread workgroup per stream.
// The encoder itself is bzip2_core.h, written against the few workgroup operations defined below; DESIGN.md section 15 has the
// specification, the work slot and the stages.
//
// Two launches per call, the kernel boundary being the fence between them:
//   prep    one workgroup: which streams are coded (length in range, slot >= bound) and where each one's work slot lies in the
//           workspace (an exclusive scan of the slots' sizes over the coded streams).
//   encode  one workgroup per stream, every stage of bzip2_core.h; no workgroup reads what another one writes.
#include "../../include/rpcc_bzip2.h"
#include "../csrc_tile/tiles.h"

static_assert(RPCC_BZIP2_ERR_ARG == TILE_ERR_ARG && RPCC_BZIP2_ERR_HIP == TILE_ERR_HIP, "rpcc_bzip2.h and tiles.h disagree");

#define BZE_FN __device__ __forceinline__
#define BZE_HD __host__ __device__ inline
#define BZE_T 1024
#define BZE_WAVE 64
#define BZE_SYNC() __syncthreads()
#define BZE_BALLOT(p) __ballot(p)
#define BZE_SHFL_UP(v, d) __shfl_up((v), (d))
#define BZE_LDS_ADD(p, v) ((void)atomicAdd((p), (v)))
#define BZE_LDS_OR(p, v) ((void)atomicOr((p), (v)))
#define BZE_LDS_XOR(p, v) ((void)atomicXor((p), (v)))
#include "bzip2_core.h"

static_assert(RPCC_BZIP2_MAX_INPUT == BZE_MAX_INPUT, "rpcc_bzip2.h and bzip2_core.h disagree");
static_assert(sizeof(BzeShared) <= 80 * 1024, "two workgroups of the encoder share a CU's 160 KB of LDS");

#define MAX_TOTAL ((int64_t)1 << 36)   // total_len of one call

extern "C" int rpcc_bzip2_version(void) { return RPCC_BZIP2_ABI_VERSION; }
extern "C" const char *rpcc_bzip2_last_error(void) { return g_err; }

// The workspace: what rpcc_bzip2_workspace_bytes sizes and rpcc_bzip2_encode carves.
struct WsLayout {
    size_t work_off, slots, slot_bytes, bytes;
};
static WsLayout ws_layout(int64_t nstreams, int64_t total_len) {
    WsLayout L;
    L.work_off = 0;                                   // int64 [nstreams]: each stream's slot, -1: the stream is not coded
    L.slots = al((size_t)nstreams * sizeof(int64_t));
    L.slot_bytes = (size_t)bze_slots_bytes(nstreams, total_len);
    L.bytes = L.slots + L.slot_bytes;
    return L;
}

__global__ __launch_bounds__(1024) void prep_kernel(const int64_t *__restrict__ src_len, const int64_t *__restrict__ dst_cap, int64_t nstreams,
                                                    int level, int64_t slot_bytes, int64_t *__restrict__ work_off, int64_t *__restrict__ dst_len) {
    __shared__ int64_t part[1024];
    __shared__ int64_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int64_t s0 = 0; s0 < nstreams; s0 += 1024) {
        const int64_t s = s0 + threadIdx.x;
        int64_t need = 0;
        if (s < nstreams) {
            const int64_t n = src_len[s];
            if (n >= 0 && n <= RPCC_BZIP2_MAX_INPUT && dst_cap[s] >= bze_bound(n, level)) need = bze_layout(bze_block_cap(n, level)).bytes;
        }
        part[threadIdx.x] = need;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {   // inclusive Hillis-Steele scan
            const int64_t y = threadIdx.x >= (unsigned)o ? part[threadIdx.x - o] : 0;
            __syncthreads();
            part[threadIdx.x] += y;
            __syncthreads();
        }
        if (s < nstreams) {
            const int64_t end = carry + part[threadIdx.x];
            const bool ok = need > 0 && end <= slot_bytes;
            work_off[s] = ok ? end - need : -1;
            if (!ok) dst_len[s] = RPCC_BZIP2_E_CAPACITY;
        }
        __syncthreads();
        if (threadIdx.x == 1023) carry += part[1023];
        __syncthreads();
    }
}

__global__ __launch_bounds__(BZE_T) void encode_kernel(const uint64_t *__restrict__ src_ptr, const int64_t *__restrict__ src_len, int level,
                                                       uint8_t *__restrict__ dst, const int64_t *__restrict__ dst_off,
                                                       const int64_t *__restrict__ dst_cap, int64_t *__restrict__ dst_len,
                                                       const int64_t *__restrict__ work_off, uint8_t *slots) {
    __shared__ BzeShared S;
    const int64_t s = blockIdx.x;
    const int64_t wo = work_off[s];
    if (wo < 0) return;
    const int64_t got = bzip2_stream(S, (int)threadIdx.x, (const uint8_t *)src_ptr[s], src_len[s], level, dst + dst_off[s], dst_cap[s], slots + wo);
    if (threadIdx.x == 0) dst_len[s] = got;
}

static bool sizes_ok(int64_t nstreams, int64_t total_len, int level) {
    return nstreams >= 0 && nstreams <= RPCC_BZIP2_MAX_STREAMS && total_len >= 0 && total_len <= MAX_TOTAL && level >= 1 && level <= 9;
}

extern "C" size_t rpcc_bzip2_bound(int64_t n, int level) { return (size_t)bze_bound(n, level); }

extern "C" size_t rpcc_bzip2_workspace_bytes(int64_t nstreams, int64_t total_len, int level) {
    return sizes_ok(nstreams, total_len, level) ? ws_layout(nstreams, total_len).bytes : 0;
}

extern "C" int rpcc_bzip2_encode(const uint64_t *src_ptr, const int64_t *src_len, int64_t nstreams, int64_t total_len, int level, uint8_t *dst,
                                 const int64_t *dst_off, const int64_t *dst_cap, int64_t *dst_len, void *ws, void *stream) {
    ARG_TRY(sizes_ok(nstreams, total_len, level));
    ARG_TRY(src_ptr && src_len && dst && dst_off && dst_cap && dst_len && ws);
    ARG_TRY(((uintptr_t)ws & 15) == 0);
    if (nstreams == 0) return 0;
    const hipStream_t st = (hipStream_t)stream;
    const WsLayout L = ws_layout(nstreams, total_len);
    int64_t *work_off = (int64_t *)((char *)ws + L.work_off);
    uint8_t *slots = (uint8_t *)ws + L.slots;
    hipLaunchKernelGGL(prep_kernel, dim3(1), dim3(1024), 0, st, src_len, dst_cap, nstreams, level, (int64_t)L.slot_bytes, work_off, dst_len);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(encode_kernel, dim3((unsigned)nstreams), dim3(BZE_T), 0, st, src_ptr, src_len, level, dst, dst_off, dst_cap, dst_len,
                       (const int64_t *)work_off, slots);
    LAUNCH_CHECK();
    return 0;
}
