// cloud_kernels.hip -- librpcc_cloud.so: a decoded batch with extra points behind every frame's image -> the rows of the .bin files
// (include/rpcc_cloud.h) for gfx950.
//
// The scheme is rows_kernels.hip's (csrc_rows/, which this library leaves alone and therefore restates): two launches with one workgroup
// per frame each, the kernel boundary the fence between them.  cloud_count_kernel counts a frame's kept pixels, its kept extra points and
// its non-zero ranges.  cloud_write_kernel sums the counts of the frames before its own, then compacts two segments one behind the other
// through the same code, cloud_segment(): the P pixels, and the frame's n = min(max(extra_count[b], 0), extra_capacity) extra points, n
// read from device memory (workgroup-uniform).  Both segments are 12-byte points -- [P,3] and [extra_capacity,3] f32 -- so a lane owns
// CLOUD_PPT consecutive points of a round, 12 consecutive dwords, in either; nothing wider than a dword is aligned.  A segment is ranked
// round by round with the wavefront DPP scan plus LDS partials, the next round's loads in flight during the scan, and every kept point
// is stored with one 16-byte store; the second segment starts at the rank the first one ended at.
//
// The choice: ONE workgroup per frame is kept, no frame is split and no third launch counts in front.  The extra segment is short beside
// the image (the 64 x 2000 example sweep hides 28 267 points behind 128 000 pixels: 7 more rounds after 32), and a chunk is 32 frames on
// 256 CUs either way; splitting a frame would buy a parallelism the image segment does not have either.  Measured on one MI355X, 256 such
// frames in chunks of 32, device events: 1.509 ms (1.508 - 1.509) for the two launches here, 122 320 rows per frame, beside 1.170 ms
// (1.163 - 1.191) for rows.pack's two on the same images, 94 053 rows per frame (tools_dev/decode_trailers_time.py; profiles/HISTORY.md).
// Both kernels decide "kept" with cloud_kept(); -ffp-contract=off keeps its sum un-fused.
#include "../../include/rpcc_cloud.h"
#include "../csrc_tile/tiles.h"

static_assert(RPCC_CLOUD_ERR_ARG == TILE_ERR_ARG && RPCC_CLOUD_ERR_HIP == TILE_ERR_HIP, "rpcc_cloud.h and tiles.h disagree");
static_assert(RPCC_CLOUD_MAX_BATCH == TILE_MAX_BATCH && RPCC_CLOUD_MAX_PIXELS == TILE_MAX_PIXELS, "rpcc_cloud.h and tiles.h disagree");

#define CLOUD_THREADS 1024   // lanes of a workgroup
#define CLOUD_PPT 4          // consecutive points of a lane per round: segment order inside a lane
#define CLOUD_WAVES (CLOUD_THREADS / 64)
static_assert(CLOUD_THREADS * CLOUD_PPT == RPCC_CLOUD_ROUND, "a round is one pass of the workgroup");

extern "C" int rpcc_cloud_version(void) { return RPCC_CLOUD_ABI_VERSION; }
extern "C" const char *rpcc_cloud_last_error(void) { return g_err; }

// the save rule: np.sum(pc, -1) != 0 over three float32 columns is this sequence; NaN compares unequal and is kept
__device__ __forceinline__ bool cloud_kept(float x, float y, float z) {
    const float s = (x + y) + z;
    return s != 0.0f;
}

struct cloud_px {
    float v[3 * CLOUD_PPT];
};

// points p0 .. p0 + CLOUD_PPT - 1 of the segment f of n points; points at or past n read as (0, 0, 0), which is not kept, and are not touched
__device__ __forceinline__ cloud_px cloud_load(const float *__restrict__ f, int p0, int n) {
    cloud_px r;
    if (p0 + CLOUD_PPT <= n) {
#pragma unroll
        for (int j = 0; j < 3 * CLOUD_PPT; j++) r.v[j] = f[3 * (size_t)p0 + j];
    } else {
#pragma unroll
        for (int j = 0; j < 3 * CLOUD_PPT; j++) r.v[j] = p0 + j / 3 < n ? f[3 * (size_t)p0 + j] : 0.0f;
    }
    return r;
}

// inclusive prefix sum over the 64 lanes: row_shr 1/2/4/8 inside each 16-lane row, then row_bcast:15 and row_bcast:31 (csrc/rpcc_device.h
// has the same six steps); all lanes must be active
__device__ __forceinline__ uint32_t cloud_wave_scan(uint32_t v) {
#define STEP_(ctrl_, rm_) v = v + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, ctrl_, rm_, 0xf, false)
    STEP_(0x111, 0xf); STEP_(0x112, 0xf); STEP_(0x114, 0xf); STEP_(0x118, 0xf); STEP_(0x142, 0xa); STEP_(0x143, 0xc);
#undef STEP_
    return v;
}

__device__ __forceinline__ long long cloud_wave_sum(long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the extra points of frame b that count: extra_count[b] clamped to 0 .. extra_capacity (workgroup-uniform); 0 without an extra segment
__device__ __forceinline__ int cloud_extra_n(const int32_t *__restrict__ extra_count, int extra_capacity, int b) {
    if (!extra_count || extra_capacity <= 0) return 0;
    const int c = extra_count[b];
    return c < 0 ? 0 : (c > extra_capacity ? extra_capacity : c);
}

// this lane's kept points of the segment f of n points
__device__ __forceinline__ uint32_t cloud_count_segment(const float *__restrict__ f, int n) {
    uint32_t kept = 0u;
    for (int r0 = 0; r0 < n; r0 += RPCC_CLOUD_ROUND) {
        const cloud_px px = cloud_load(f, r0 + (int)threadIdx.x * CLOUD_PPT, n);
#pragma unroll
        for (int k = 0; k < CLOUD_PPT; k++) kept += cloud_kept(px.v[3 * k], px.v[3 * k + 1], px.v[3 * k + 2]) ? 1u : 0u;
    }
    return kept;
}

// counts[b] = the frame's kept pixels + kept extra points; nonzero[b] = its pixels with ri != 0
__global__ __launch_bounds__(CLOUD_THREADS) void cloud_count_kernel(const float *__restrict__ pc, const float *__restrict__ ri, int P,
                                                                   const float *__restrict__ extra, int extra_capacity,
                                                                   const int32_t *__restrict__ extra_count, int64_t *__restrict__ counts,
                                                                   int32_t *__restrict__ nonzero) {
    __shared__ uint32_t s_kept[CLOUD_WAVES], s_nz[CLOUD_WAVES];
    const int b = blockIdx.x;
    const int n = cloud_extra_n(extra_count, extra_capacity, b);
    uint32_t kept = cloud_count_segment(pc + 3 * (size_t)b * P, P), nz = 0u;
    if (n > 0) kept += cloud_count_segment(extra + 3 * (size_t)b * extra_capacity, n);
    if (nonzero)
        for (int p = threadIdx.x; p < P; p += CLOUD_THREADS) nz += ri[(size_t)b * P + p] != 0.0f ? 1u : 0u;
    kept = (uint32_t)cloud_wave_sum(kept), nz = (uint32_t)cloud_wave_sum(nz);
    if ((threadIdx.x & 63) == 0) s_kept[threadIdx.x >> 6] = kept, s_nz[threadIdx.x >> 6] = nz;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t a = 0u, m = 0u;
        for (int w = 0; w < CLOUD_WAVES; w++) a += s_kept[w], m += s_nz[w];
        counts[b] = a;
        if (nonzero) nonzero[b] = (int32_t)m;
    }
}

// One segment of a frame: the kept points of f[0 .. n) become rows out[running ..], in order; w4 the fourth column or nullptr (+0.0).
// room: the rows `out` may hold -- >= the frame's rows, so a rank at or past it is never stored.  wsum: CLOUD_WAVES words of LDS.
// Called by every lane of the workgroup with the same f, n, w4, out, room, running (workgroup-uniform).  -> running + the segment's rows.
__device__ __forceinline__ uint32_t cloud_segment(const float *__restrict__ f, int n, const float *__restrict__ w4, float4 *__restrict__ out,
                                                  long long room, uint32_t running, uint32_t *wsum) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    cloud_px px = cloud_load(f, (int)threadIdx.x * CLOUD_PPT, n);
    for (int r0 = 0; r0 < n; r0 += RPCC_CLOUD_ROUND) {   // (workgroup-uniform)
        const int p0 = r0 + (int)threadIdx.x * CLOUD_PPT;
        const cloud_px nxt = cloud_load(f, p0 + RPCC_CLOUD_ROUND, n);   // the next round's points are on their way during the scan
        bool keep[CLOUD_PPT];
        uint32_t cnt = 0u;
#pragma unroll
        for (int k = 0; k < CLOUD_PPT; k++) {
            keep[k] = p0 + k < n && cloud_kept(px.v[3 * k], px.v[3 * k + 1], px.v[3 * k + 2]);
            cnt += keep[k] ? 1u : 0u;
        }
        const uint32_t incl = cloud_wave_scan(cnt);
        __syncthreads();   // (wsum of the round -- or the segment -- before has been read)
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        uint32_t rank = running + incl - cnt, total = 0u;
#pragma unroll
        for (int w = 0; w < CLOUD_WAVES; w++) {
            const uint32_t s = wsum[w];
            rank += w < wave ? s : 0u;
            total += s;
        }
#pragma unroll
        for (int k = 0; k < CLOUD_PPT; k++) {
            if (keep[k] && (long long)rank < room) {
                out[rank] = make_float4(px.v[3 * k], px.v[3 * k + 1], px.v[3 * k + 2], w4 ? w4[p0 + k] : 0.0f);
                rank++;
            }
        }
        running += total;
        px = nxt;
    }
    return running;
}

// table: RPCC_CLOUD_TABLE_WORDS(B) words, the counts in its tail (written by the launch before); the offsets and the status are written here
__global__ __launch_bounds__(CLOUD_THREADS) void cloud_write_kernel(const float *__restrict__ pc, const float *__restrict__ inten, int B, int P,
                                                                   float4 *__restrict__ rows, int64_t cap, int64_t *__restrict__ table,
                                                                   const int64_t *__restrict__ base, const float *__restrict__ extra,
                                                                   int extra_capacity, const int32_t *__restrict__ extra_count) {
    __shared__ long long s_sum[2][CLOUD_WAVES];
    __shared__ uint32_t wsum[CLOUD_WAVES];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t *__restrict__ counts = table + B + 2;
    long long before = 0, all = 0;
    for (int i = threadIdx.x; i < B; i += CLOUD_THREADS) {
        const long long c = counts[i];
        all += c;
        before += i < b ? c : 0;
    }
    before = cloud_wave_sum(before), all = cloud_wave_sum(all);
    if (lane == 0) s_sum[0][wave] = before, s_sum[1][wave] = all;
    __syncthreads();
    const long long start = base ? *base : 0;
    before = start, all = start;
    for (int w = 0; w < CLOUD_WAVES; w++) before += s_sum[0][w], all += s_sum[1][w];
    const bool fits = start >= 0 && all <= cap;   // (workgroup-uniform, and the same in every workgroup)
    if (threadIdx.x == 0) {
        table[b + 1] = before + counts[b];
        if (b == 0) table[0] = start, table[B + 1] = fits ? RPCC_CLOUD_OK : RPCC_CLOUD_E_CAPACITY;
    }
    if (!fits) return;
    float4 *__restrict__ out = rows + before;
    const long long room = cap - before;
    const uint32_t pixels = cloud_segment(pc + 3 * (size_t)b * P, P, inten ? inten + (size_t)b * P : nullptr, out, room, 0u, wsum);
    const int n = cloud_extra_n(extra_count, extra_capacity, b);
    if (n > 0) cloud_segment(extra + 3 * (size_t)b * extra_capacity, n, nullptr, out, room, pixels, wsum);
}

extern "C" int rpcc_cloud_pack(const float *pc, const float *intensity, const float *ri_rec, int B, int P, float *rows, int64_t rows_capacity,
                               int64_t *offsets, int32_t *nonzero, const int64_t *base, const float *extra, int extra_capacity,
                               const int32_t *extra_count, void *stream) {
    ARG_TRY(B >= 1 && B <= RPCC_CLOUD_MAX_BATCH && P >= 1 && P <= RPCC_CLOUD_MAX_PIXELS);
    ARG_TRY(extra_capacity >= 0 && extra_capacity <= RPCC_CLOUD_MAX_PIXELS);
    ARG_TRY((long long)B * ((long long)P + extra_capacity) < (1ll << 31));
    ARG_TRY(pc && offsets && rows_capacity >= 0 && (rows || rows_capacity == 0));
    ARG_TRY(!nonzero || ri_rec);
    ARG_TRY(!extra || extra_count);
    ARG_TRY((uintptr_t)rows % 16 == 0 && (uintptr_t)offsets % 8 == 0 && (uintptr_t)base % 8 == 0);
    ARG_TRY((uintptr_t)pc % 4 == 0 && (uintptr_t)intensity % 4 == 0 && (uintptr_t)ri_rec % 4 == 0 && (uintptr_t)nonzero % 4 == 0);
    ARG_TRY((uintptr_t)extra % 4 == 0 && (uintptr_t)extra_count % 4 == 0);
    if (!extra) extra_capacity = 0, extra_count = nullptr;
    hipStream_t st = (hipStream_t)stream;
    cloud_count_kernel<<<B, CLOUD_THREADS, 0, st>>>(pc, ri_rec, P, extra, extra_capacity, extra_count, offsets + B + 2, nonzero);
    LAUNCH_CHECK();
    cloud_write_kernel<<<B, CLOUD_THREADS, 0, st>>>(pc, intensity, B, P, (float4 *)rows, rows_capacity, offsets, base, extra, extra_capacity,
                                                   extra_count);
    LAUNCH_CHECK();
    return 0;
}
