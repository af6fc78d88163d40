// tiles.h -- what librpcc_eval.so (csrc_eval/) and librpcc_seg.so (csrc_seg/) share: the error state of their C entries, the
// fp32 distance and its tile bound, and the preparation of a batch of H x W images cut into 8x32-pixel tiles (tile boxes, row
// counts, per-frame scans).  Each library includes it once, so each .so keeps its own copy of the static state below.
#ifndef RPCC_TILES_H
#define RPCC_TILES_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>

#define TILE_R 8        // tile rows
#define TILE_C 32       // tile columns (8 x 32 = 256 pixels, one per lane: the FPS tile of fps_kernels.h)
#define TILE_LIST 1024  // tiles kept per round of a search's tile list (any table size: the rounds cover it)

// The libraries' own headers define the same values (RPCC_EVAL_*, RPCC_SEG_*); each asserts that they match.
#define TILE_ERR_ARG (-1)
#define TILE_ERR_HIP (-2)
#define TILE_MAX_BATCH 65535       // frames per call: the frame index is a grid dimension
#define TILE_MAX_PIXELS (1 << 26)  // H*W per frame

static thread_local char g_err[512] = "";
static int set_err(int code, const char *fmt, const char *a = "", const char *b = "") {
    snprintf(g_err, sizeof(g_err), fmt, a, b);
    return code;
}
#define HIP_TRY(expr)                                                                               \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess) return set_err(TILE_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)
#define ARG_TRY(cond)                                                             \
    do {                                                                          \
        if (!(cond)) return set_err(TILE_ERR_ARG, "bad argument: %s%s", #cond); \
    } while (0)
#define LAUNCH_CHECK() HIP_TRY(hipGetLastError())

// ------------------------------------------------------------------------------------------------
// device helpers
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float dist3(float ax, float ay, float az, float bx, float by, float bz) {
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    return ((dx * dx) + (dy * dy)) + (dz * dz);
}

// Lower bound of dist3 between any point of box Q = [qlo, qhi] and any point of box S = [lo, hi] (a query point: qlo = qhi).
// Per axis the gap is ONE rounded subtraction of box faces: for q in Q and p in S with qhi < lo, q - p <= qhi - lo < 0, and
// rounding is monotone, so |fl(q - p)| >= fl(lo - qhi); likewise fl(qlo - hi) when qlo > hi; 0 when the extents overlap.
// Squares and the two sums are monotone in their (non-negative) operands and are evaluated in the same order as dist3, so
// bound <= dist3(q, p) for every pair, bit for bit.
__device__ __forceinline__ float box_bound(float3 qlo, float3 qhi, float4 lo, float4 hi) {
    const float gx = fmaxf(fmaxf(lo.x - qhi.x, qlo.x - hi.x), 0.f);
    const float gy = fmaxf(fmaxf(lo.y - qhi.y, qlo.y - hi.y), 0.f);
    const float gz = fmaxf(fmaxf(lo.z - qhi.z, qlo.z - hi.z), 0.f);
    return ((gx * gx) + (gy * gy)) + (gz * gz);
}

__device__ __forceinline__ float wave_min(float v) {
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// Exclusive scan of one flag per thread over a 256-thread block; returns the flag's offset, *total = the block's count.
__device__ __forceinline__ int block_scan_flag(bool f, int *s_w, int *total) {
    const unsigned long long m = __ballot(f);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int in_wave = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) s_w[w] = __popcll(m);
    __syncthreads();
    int off = 0;
    for (int k = 0; k < w; ++k) off += s_w[k];
    *total = s_w[0] + s_w[1] + s_w[2] + s_w[3];
    __syncthreads();
    return off + in_wave;
}

// ------------------------------------------------------------------------------------------------
// preparation kernels
// ------------------------------------------------------------------------------------------------
// Per tile: the box of its points and their count, tiles[b][t] = (lo.xyz, count as int bits), (hi.xyz, 0).
// ld(i, p) reads pixel i of the batch (b*H*W + row*W + col) into p and returns whether it holds a point.
template <class Load>
__global__ __launch_bounds__(256) void tile_box_kernel(Load ld, int H, int W, int ntc, int T, float4 *__restrict__ tiles) {
    const int t = blockIdx.x, b = blockIdx.y;
    const size_t P = (size_t)H * W;
    const int row = (t / ntc) * TILE_R + (threadIdx.x >> 5), col = (t % ntc) * TILE_C + (threadIdx.x & 31);
    float3 p = make_float3(0.f, 0.f, 0.f);
    const bool v = row < H && col < W && ld((size_t)b * P + (size_t)row * W + col, p);
    float lx = v ? p.x : INFINITY, ly = v ? p.y : INFINITY, lz = v ? p.z : INFINITY;
    float hx = v ? p.x : -INFINITY, hy = v ? p.y : -INFINITY, hz = v ? p.z : -INFINITY;
    lx = wave_min(lx), ly = wave_min(ly), lz = wave_min(lz);
    hx = wave_max(hx), hy = wave_max(hy), hz = wave_max(hz);
    const int cnt = __popcll(__ballot(v));
    __shared__ float s[4][6];
    __shared__ int sc[4];
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        s[w][0] = lx, s[w][1] = ly, s[w][2] = lz, s[w][3] = hx, s[w][4] = hy, s[w][5] = hz;
        sc[w] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 4; ++k) {
            lx = fminf(lx, s[k][0]), ly = fminf(ly, s[k][1]), lz = fminf(lz, s[k][2]);
            hx = fmaxf(hx, s[k][3]), hy = fmaxf(hy, s[k][4]), hz = fmaxf(hz, s[k][5]);
        }
        float4 *o = tiles + ((size_t)b * T + t) * 2;
        o[0] = make_float4(lx, ly, lz, __int_as_float(sc[0] + sc[1] + sc[2] + sc[3]));
        o[1] = make_float4(hx, hy, hz, 0.f);
    }
}

// Per row: the pixels for which is_point(b, h, x, H, W) holds -> rowcnt[b][h].
template <class Pred>
__global__ __launch_bounds__(256) void row_count_kernel(Pred is_point, int H, int W, int32_t *__restrict__ rowcnt) {
    const int h = blockIdx.x, b = blockIdx.y;
    int c = 0;
    // The predicate's pointers come from a struct and carry no noalias: left alone, the vectoriser interleaves seg's fp64 test
    // 8-fold (142 VGPRs instead of 34) in this load-bound loop.
#pragma clang loop interleave_count(1)
    for (int x = threadIdx.x; x < W; x += 256) c += is_point(b, h, x, H, W) ? 1 : 0;
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    __shared__ int s[4];
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) rowcnt[(size_t)b * H + h] = s[0] + s[1] + s[2] + s[3];
}

// One workgroup per frame: exclusive prefix of the frame's len counts, and their total to total[STRIDE * b].
template <int STRIDE>
__global__ __launch_bounds__(256) void scan_kernel(const int32_t *__restrict__ cnt, int len, int32_t *__restrict__ off,
                                                   int32_t *__restrict__ total) {
    const int b = blockIdx.x;
    __shared__ int s_v[256];
    int base = 0;
    for (int h0 = 0; h0 < len; h0 += 256) {
        const int h = h0 + threadIdx.x;
        const int v = h < len ? cnt[(size_t)b * len + h] : 0;
        s_v[threadIdx.x] = v;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {   // Hillis-Steele inclusive scan
            const int a = threadIdx.x >= o ? s_v[threadIdx.x - o] : 0;
            __syncthreads();
            s_v[threadIdx.x] += a;
            __syncthreads();
        }
        if (h < len) off[(size_t)b * len + h] = base + s_v[threadIdx.x] - v;
        base += s_v[255];
        __syncthreads();
    }
    if (threadIdx.x == 0) total[STRIDE * b] = base;
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
static size_t al(size_t x) { return (x + 255) & ~(size_t)255; }

static bool shape_ok(int B, int H, int W) {
    return B > 0 && B <= TILE_MAX_BATCH && H > 0 && W > 0 && (long long)H * W <= TILE_MAX_PIXELS;
}

static int tile_cols(int W) { return (W + TILE_C - 1) / TILE_C; }
static int tile_count(int H, int W) { return ((H + TILE_R - 1) / TILE_R) * tile_cols(W); }

#endif  // RPCC_TILES_H
