// rows_kernels.hip -- librpcc_rows.so: a decoded batch -> the rows of the .bin files (include/rpcc_rows.h) for gfx950.
//
// Two launches with one workgroup per frame each; the kernel boundary is the fence between them (nothing is published
// between workgroups of one launch).  rows_count_kernel counts a frame's kept pixels and non-zero ranges.  rows_write_kernel sums the
// counts of the frames before its own -- B is small --, ranks its pixels round by round with the wavefront DPP scan plus LDS partials (the
// scheme of intensity_pack_kernel, csrc/intensity_kernels.h) and stores every kept row with one 16-byte store.  A lane owns ROWS_PPT
// consecutive pixels of a round, 12 consecutive dwords of pc: frames start at 12 * P * b bytes, so nothing wider than a dword is aligned.
// Both kernels decide "kept" with rows_kept(); -ffp-contract=off keeps its sum un-fused.
#include "../../include/rpcc_rows.h"
#include "../csrc_tile/tiles.h"

static_assert(RPCC_ROWS_ERR_ARG == TILE_ERR_ARG && RPCC_ROWS_ERR_HIP == TILE_ERR_HIP, "rpcc_rows.h and tiles.h disagree");
static_assert(RPCC_ROWS_MAX_BATCH == TILE_MAX_BATCH && RPCC_ROWS_MAX_PIXELS == TILE_MAX_PIXELS, "rpcc_rows.h and tiles.h disagree");

#define ROWS_THREADS 1024   // lanes of a workgroup
#define ROWS_PPT 4          // consecutive pixels of a lane per round: raster order inside a lane
#define ROWS_WAVES (ROWS_THREADS / 64)
static_assert(ROWS_THREADS * ROWS_PPT == RPCC_ROWS_ROUND, "a round is one pass of the workgroup");

extern "C" int rpcc_rows_version(void) { return RPCC_ROWS_ABI_VERSION; }
extern "C" const char *rpcc_rows_last_error(void) { return g_err; }

// the save rule: np.sum(pc, -1) != 0 over three float32 columns is this sequence; NaN compares unequal and is kept
__device__ __forceinline__ bool rows_kept(float x, float y, float z) {
    const float s = (x + y) + z;
    return s != 0.0f;
}

struct rows_px {
    float v[3 * ROWS_PPT];
};

// pixels p0 .. p0 + ROWS_PPT - 1 of the frame f; pixels at or past P read as (0, 0, 0), which is not kept
__device__ __forceinline__ rows_px rows_load(const float *__restrict__ f, int p0, int P) {
    rows_px r;
    if (p0 + ROWS_PPT <= P) {
#pragma unroll
        for (int j = 0; j < 3 * ROWS_PPT; j++) r.v[j] = f[3 * (size_t)p0 + j];
    } else {
#pragma unroll
        for (int j = 0; j < 3 * ROWS_PPT; j++) r.v[j] = p0 + j / 3 < P ? f[3 * (size_t)p0 + j] : 0.0f;
    }
    return r;
}

// inclusive prefix sum over the 64 lanes: row_shr 1/2/4/8 inside each 16-lane row, then row_bcast:15 and row_bcast:31 (csrc/rpcc_device.h
// has the same six steps); all lanes must be active
__device__ __forceinline__ uint32_t rows_wave_scan(uint32_t v) {
#define STEP_(ctrl_, rm_) v = v + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, ctrl_, rm_, 0xf, false)
    STEP_(0x111, 0xf); STEP_(0x112, 0xf); STEP_(0x114, 0xf); STEP_(0x118, 0xf); STEP_(0x142, 0xa); STEP_(0x143, 0xc);
#undef STEP_
    return v;
}

__device__ __forceinline__ long long rows_wave_sum(long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// counts[b] = the frame's kept pixels; nonzero[b] = its pixels with ri != 0
__global__ __launch_bounds__(ROWS_THREADS) void rows_count_kernel(const float *__restrict__ pc, const float *__restrict__ ri, int P,
                                                                 int64_t *__restrict__ counts, int32_t *__restrict__ nonzero) {
    __shared__ uint32_t s_kept[ROWS_WAVES], s_nz[ROWS_WAVES];
    const int b = blockIdx.x;
    const float *__restrict__ f = pc + 3 * (size_t)b * P;
    uint32_t kept = 0u, nz = 0u;
    for (int r0 = 0; r0 < P; r0 += RPCC_ROWS_ROUND) {
        const rows_px px = rows_load(f, r0 + (int)threadIdx.x * ROWS_PPT, P);
#pragma unroll
        for (int k = 0; k < ROWS_PPT; k++) kept += rows_kept(px.v[3 * k], px.v[3 * k + 1], px.v[3 * k + 2]) ? 1u : 0u;
    }
    if (nonzero)
        for (int p = threadIdx.x; p < P; p += ROWS_THREADS) nz += ri[(size_t)b * P + p] != 0.0f ? 1u : 0u;
    kept = (uint32_t)rows_wave_sum(kept), nz = (uint32_t)rows_wave_sum(nz);
    if ((threadIdx.x & 63) == 0) s_kept[threadIdx.x >> 6] = kept, s_nz[threadIdx.x >> 6] = nz;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t a = 0u, n = 0u;
        for (int w = 0; w < ROWS_WAVES; w++) a += s_kept[w], n += s_nz[w];
        counts[b] = a;
        if (nonzero) nonzero[b] = (int32_t)n;
    }
}

// table: RPCC_ROWS_TABLE_WORDS(B) words, the counts in its tail (written by the launch before); the offsets and the status are written here
__global__ __launch_bounds__(ROWS_THREADS) void rows_write_kernel(const float *__restrict__ pc, const float *__restrict__ inten, int B, int P,
                                                                 float4 *__restrict__ rows, int64_t cap, int64_t *__restrict__ table,
                                                                 const int64_t *__restrict__ base) {
    __shared__ long long s_sum[2][ROWS_WAVES];
    __shared__ uint32_t wsum[ROWS_WAVES];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t *__restrict__ counts = table + B + 2;
    long long before = 0, all = 0;
    for (int i = threadIdx.x; i < B; i += ROWS_THREADS) {
        const long long c = counts[i];
        all += c;
        before += i < b ? c : 0;
    }
    before = rows_wave_sum(before), all = rows_wave_sum(all);
    if (lane == 0) s_sum[0][wave] = before, s_sum[1][wave] = all;
    __syncthreads();
    const long long start = base ? *base : 0;
    before = start, all = start;
    for (int w = 0; w < ROWS_WAVES; w++) before += s_sum[0][w], all += s_sum[1][w];
    const bool fits = start >= 0 && all <= cap;   // (workgroup-uniform, and the same in every workgroup)
    if (threadIdx.x == 0) {
        table[b + 1] = before + counts[b];
        if (b == 0) table[0] = start, table[B + 1] = fits ? RPCC_ROWS_OK : RPCC_ROWS_E_CAPACITY;
    }
    if (!fits) return;
    const float *__restrict__ f = pc + 3 * (size_t)b * P;
    const float *__restrict__ w4 = inten ? inten + (size_t)b * P : nullptr;
    float4 *__restrict__ out = rows + before;
    const long long room = cap - before;   // >= the frame's rows: a rank at or past it is never stored
    uint32_t running = 0u;
    rows_px px = rows_load(f, (int)threadIdx.x * ROWS_PPT, P);
    for (int r0 = 0; r0 < P; r0 += RPCC_ROWS_ROUND) {   // (workgroup-uniform)
        const int p0 = r0 + (int)threadIdx.x * ROWS_PPT;
        const rows_px nxt = rows_load(f, p0 + RPCC_ROWS_ROUND, P);   // the next round's pixels are on their way during the scan
        bool keep[ROWS_PPT];
        uint32_t cnt = 0u;
#pragma unroll
        for (int k = 0; k < ROWS_PPT; k++) {
            keep[k] = p0 + k < P && rows_kept(px.v[3 * k], px.v[3 * k + 1], px.v[3 * k + 2]);
            cnt += keep[k] ? 1u : 0u;
        }
        const uint32_t incl = rows_wave_scan(cnt);
        __syncthreads();   // (wsum of the round before has been read)
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        uint32_t rank = running + incl - cnt, total = 0u;
#pragma unroll
        for (int w = 0; w < ROWS_WAVES; w++) {
            const uint32_t s = wsum[w];
            rank += w < wave ? s : 0u;
            total += s;
        }
#pragma unroll
        for (int k = 0; k < ROWS_PPT; k++) {
            if (keep[k] && (long long)rank < room) {
                out[rank] = make_float4(px.v[3 * k], px.v[3 * k + 1], px.v[3 * k + 2], w4 ? w4[p0 + k] : 0.0f);
                rank++;
            }
        }
        running += total;
        px = nxt;
    }
}

extern "C" int rpcc_rows_pack(const float *pc, const float *intensity, const float *ri_rec, int B, int P, float *rows, int64_t rows_capacity,
                              int64_t *offsets, int32_t *nonzero, const int64_t *base, void *stream) {
    ARG_TRY(B >= 1 && B <= RPCC_ROWS_MAX_BATCH && P >= 1 && P <= RPCC_ROWS_MAX_PIXELS);
    ARG_TRY((long long)B * P < (1ll << 31));
    ARG_TRY(pc && offsets && rows_capacity >= 0 && (rows || rows_capacity == 0));
    ARG_TRY(!nonzero || ri_rec);
    ARG_TRY((uintptr_t)rows % 16 == 0 && (uintptr_t)offsets % 8 == 0 && (uintptr_t)base % 8 == 0);
    ARG_TRY((uintptr_t)pc % 4 == 0 && (uintptr_t)intensity % 4 == 0 && (uintptr_t)ri_rec % 4 == 0 && (uintptr_t)nonzero % 4 == 0);
    hipStream_t st = (hipStream_t)stream;
    rows_count_kernel<<<B, ROWS_THREADS, 0, st>>>(pc, ri_rec, P, offsets + B + 2, nonzero);
    LAUNCH_CHECK();
    rows_write_kernel<<<B, ROWS_THREADS, 0, st>>>(pc, intensity, B, P, (float4 *)rows, rows_capacity, offsets, base);
    LAUNCH_CHECK();
    return 0;
}
