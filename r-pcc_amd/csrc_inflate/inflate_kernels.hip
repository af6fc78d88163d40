// inflate_kernels.hip -- librpcc_inflate.so (include/rpcc_inflate.h): gzip members decoded on gfx950, one wavefront per stream.
// The decoder itself is inflate_core.h, written against the few wave operations defined below; DESIGN.md section 13 has the format,
// the statuses, the kernel and its LDS budget.  The ring copy of the LZ4 decoder and the CRC-32 fold of the deflate encoder are
// written again here on purpose: the three entropy libraries share no decoder code.
#include "../../include/rpcc_inflate.h"
#include "../csrc_tile/tiles.h"

static_assert(RPCC_INFLATE_ERR_ARG == TILE_ERR_ARG && RPCC_INFLATE_ERR_HIP == TILE_ERR_HIP, "rpcc_inflate.h and tiles.h disagree");

#define INF_FN __device__ __forceinline__
#define INF_CONST static __device__ const
#define INF_WAVE 64
#define INF_SYNC() __syncthreads()
#define INF_UNI(x) __builtin_amdgcn_readfirstlane((int)(x))
#define INF_BALLOT(p) __ballot(p)
#define INF_SHFL_XOR(v, m) __shfl_xor((v), (m))
#define INF_BREV(x) __brev(x)
#include "inflate_core.h"

static_assert(sizeof(InfShared) <= 40 * 1024, "four waves of the decoder share a CU's 160 KB of LDS");

extern "C" int rpcc_inflate_version(void) { return RPCC_INFLATE_ABI_VERSION; }
extern "C" const char *rpcc_inflate_last_error(void) { return g_err; }

__global__ __launch_bounds__(64) void inflate_kernel(const uint64_t *__restrict__ src_ptr, const int64_t *__restrict__ src_len,
                                                     uint8_t *__restrict__ dst, const int64_t *__restrict__ dst_off,
                                                     const int64_t *__restrict__ dst_cap, int64_t *__restrict__ dst_len,
                                                     int32_t *__restrict__ status) {
    __shared__ InfShared S;
    const int64_t s = blockIdx.x;
    int64_t produced = 0;
    const int st = inflate_stream(S, (int)threadIdx.x, (const uint8_t *)src_ptr[s], src_len[s], dst + dst_off[s], dst_cap[s], produced);
    if (threadIdx.x == 0) {
        status[s] = st;
        dst_len[s] = produced;
    }
}

extern "C" int rpcc_inflate_decode(const uint64_t *src_ptr, const int64_t *src_len, int64_t nstreams, uint8_t *dst, const int64_t *dst_off,
                                   const int64_t *dst_cap, int64_t *dst_len, int32_t *status, void *stream) {
    ARG_TRY(nstreams >= 0 && nstreams <= RPCC_INFLATE_MAX_STREAMS);
    ARG_TRY(src_ptr && src_len && dst && dst_off && dst_cap && dst_len && status);
    if (nstreams == 0) return 0;
    hipLaunchKernelGGL(inflate_kernel, dim3((unsigned)nstreams), dim3(64), 0, (hipStream_t)stream, src_ptr, src_len, dst, dst_off, dst_cap,
                       dst_len, status);
    LAUNCH_CHECK();
    return 0;
}
