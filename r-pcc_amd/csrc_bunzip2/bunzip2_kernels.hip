// bunzip2_kernels.hip -- librpcc_bunzip2.so (include/rpcc_bunzip2.h): bzip2 streams decoded on gfx950, one wavefront per stream.
// The decoder itself is bunzip2_core.h, written against the few wave operations defined below; DESIGN.md section 14 has the format,
// the statuses, the kernel's stages and its LDS and work budget.  The input window and the CRC fold of the inflate decoder are written
// again here on purpose: the entropy libraries share no decoder code.
#include "../../include/rpcc_bunzip2.h"
#include "../csrc_tile/tiles.h"

static_assert(RPCC_BUNZIP2_ERR_ARG == TILE_ERR_ARG && RPCC_BUNZIP2_ERR_HIP == TILE_ERR_HIP, "rpcc_bunzip2.h and tiles.h disagree");

#define BZ_FN __device__ __forceinline__
#define BZ_HD __host__ __device__ inline
#define BZ_WAVE 64
#define BZ_SYNC() __syncthreads()
#define BZ_UNI(x) __builtin_amdgcn_readfirstlane((int)(x))
#define BZ_BALLOT(p) __ballot(p)
#define BZ_SHFL_XOR(v, m) __shfl_xor((v), (m))
#define BZ_SHFL_UP(v, d) __shfl_up((v), (d))
#define BZ_READLANE(v, l) __builtin_amdgcn_readlane((int)(v), (l))
#define BZ_LDS_ADD(p, v) ((void)atomicAdd((p), (v)))
#define BZ_LDS_FETCH_ADD(p, v) atomicAdd((p), (v))
#include "bunzip2_core.h"

static_assert(sizeof(BzShared) <= 40 * 1024, "four waves of the decoder share a CU's 160 KB of LDS");

extern "C" int rpcc_bunzip2_version(void) { return RPCC_BUNZIP2_ABI_VERSION; }
extern "C" const char *rpcc_bunzip2_last_error(void) { return g_err; }

extern "C" int64_t rpcc_bunzip2_stream_work_bytes(int64_t nblock_max) {
    ARG_TRY(nblock_max >= 0);
    return bz_work_layout(nblock_max < RPCC_BUNZIP2_MAX_BLOCK ? nblock_max : RPCC_BUNZIP2_MAX_BLOCK).bytes;
}

__global__ __launch_bounds__(64) void bunzip2_kernel(const uint64_t *__restrict__ src_ptr, const int64_t *__restrict__ src_len,
                                                     uint8_t *__restrict__ dst, const int64_t *__restrict__ dst_off,
                                                     const int64_t *__restrict__ dst_cap, uint8_t *work, const int64_t *__restrict__ work_off,
                                                     const int64_t *__restrict__ work_cap, int64_t *__restrict__ dst_len,
                                                     int64_t *__restrict__ src_used, int32_t *__restrict__ status) {
    __shared__ BzShared S;
    const int64_t s = blockIdx.x;
    int64_t produced = 0, used = 0;
    const int64_t cap = dst_cap[s] > 0 ? dst_cap[s] : 0, wcap = work_cap[s] > 0 ? work_cap[s] : 0;
    const int st = bunzip2_stream(S, (int)threadIdx.x, (const uint8_t *)src_ptr[s], src_len[s], dst + dst_off[s], cap, work + work_off[s], wcap,
                                  produced, used);
    if (threadIdx.x == 0) {
        status[s] = st;
        dst_len[s] = produced;
        src_used[s] = used;
    }
}

extern "C" int rpcc_bunzip2_decode(const uint64_t *src_ptr, const int64_t *src_len, int64_t nstreams, uint8_t *dst, const int64_t *dst_off,
                                   const int64_t *dst_cap, uint8_t *work, const int64_t *work_off, const int64_t *work_cap, int64_t *dst_len,
                                   int64_t *src_used, int32_t *status, void *stream) {
    ARG_TRY(nstreams >= 0 && nstreams <= RPCC_BUNZIP2_MAX_STREAMS);
    ARG_TRY(src_ptr && src_len && dst && dst_off && dst_cap && work && work_off && work_cap && dst_len && src_used && status);
    if (nstreams == 0) return 0;
    hipLaunchKernelGGL(bunzip2_kernel, dim3((unsigned)nstreams), dim3(64), 0, (hipStream_t)stream, src_ptr, src_len, dst, dst_off, dst_cap,
                       work, work_off, work_cap, dst_len, src_used, status);
    LAUNCH_CHECK();
    return 0;
}
