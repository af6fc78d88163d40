// radius_filter.hip -- librpcc_filter.so: radius outlier removal (include/rpcc_filter.h) for gfx950.
//
// A tile is 256 consecutive points of ONE frame's list (the last tile of a frame is partial, no tile straddles two frames).  The
// host knows only B and total, so every grid covers NT = total / 256 + B tiles, an upper bound of sum ceil(n_b / 256); the tiles a
// batch does not use return at once.
//   frames_kernel   one workgroup: the first tile of every frame (an exclusive scan of ceil(n_b / 256)); zeroes kept and stats.
//   box_kernel      one workgroup per tile: its frame (a binary search of the scan), the box of its FINITE points and their count.
//   search_kernel   one workgroup per query tile, one point per lane: the tile itself first, then rounds of candidate tiles whose
//                   box_bound against the box of the lanes still short of nb_points + 1 neighbours does not exceed the screen's upper
//                   threshold, each staged in LDS -- unless no single lane's own bound lets it in.  A lane stops counting at
//                   nb_points + 1, the workgroup when no lane needs more.
// The clipped count min(neighbours, nb_points + 1) does not depend on the order anything is visited in, and a tile is skipped only
// when its bound proves that it holds no neighbour, so pruned and brute-force results are equal bit for bit.  Workgroups publish
// nothing to each other inside a launch (kept and stats are integer sums); the kernel boundaries are the fences.
#include "../../include/rpcc_filter.h"
#include "../csrc_tile/tiles.h"

static_assert(RPCC_FILTER_ERR_ARG == TILE_ERR_ARG && RPCC_FILTER_ERR_HIP == TILE_ERR_HIP && RPCC_FILTER_MAX_BATCH == TILE_MAX_BATCH,
              "rpcc_filter.h and tiles.h disagree");
static_assert(RPCC_FILTER_TILE == 256 && RPCC_FILTER_TILE_LIST == 256, "one point and one candidate tile per lane of a 256-thread workgroup");

#define FT RPCC_FILTER_TILE

extern "C" int rpcc_filter_version(void) { return RPCC_FILTER_ABI_VERSION; }
extern "C" const char *rpcc_filter_last_error(void) { return g_err; }

// ------------------------------------------------------------------------------------------------
// the neighbour test
// ------------------------------------------------------------------------------------------------
// Exact rule: ((dx*dx) + (dy*dy)) + (dz*dz) < radius*radius in fp64, un-fused, dx = double(xp) - double(xq).
__device__ __forceinline__ bool exact_nb(float px, float py, float pz, float qx, float qy, float qz, double r2) {
    const double dx = (double)px - (double)qx, dy = (double)py - (double)qy, dz = (double)pz - (double)qz;
    return ((dx * dx) + (dy * dy)) + (dz * dz) < r2;
}

// fp32 screen, restated from search_kernel of librpcc_seg.so: the derivation stands at screen_nb in csrc_seg/dbscan_kernels.hip
// (d2f lies within (1 +- u)^5 of the real squared distance, u = 2^-24, so d2f < r^2 (1 - 8u) is a neighbour, d2f > r^2 (1 + 8u) is
// not, and the band between gets the exact test; lo / hi are those bounds rounded inwards on the host, screen_bounds below; the
// entry checks 1e-30 <= r^2 <= 1e30 for the underflow term).  Both points are finite here, so d2f is never NaN; +inf is above hi.
__device__ __forceinline__ bool screen_nb(float px, float py, float pz, float qx, float qy, float qz, float lo, float hi, double r2) {
    const float d = dist3(px, py, pz, qx, qy, qz);
    if (d < lo) return true;
    if (d > hi) return false;
    return exact_nb(px, py, pz, qx, qy, qz, r2);
}

__device__ __forceinline__ bool finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// ------------------------------------------------------------------------------------------------
// frames and tiles
// ------------------------------------------------------------------------------------------------
struct FilterArgs {
    const char *pts;          // points, stride bytes apart
    int stride;               // 12 or 16
    const int64_t *offsets;   // [B+1]
    int64_t total;
    int B;
    const int32_t *tbase;     // [B+1] first tile of every frame, tbase[B] = tiles in use (<= NT)
    const int32_t *tframe;    // [NT] frame of a tile, -1: not in use
    const float4 *boxes;      // [NT,2] (lo.xyz, finite points as int bits), (hi.xyz, 0)
};

// Frame b's points: [*start, *start + n), both ends clamped into 0 .. total.
__device__ __forceinline__ int64_t frame_range(const int64_t *offsets, int b, int64_t total, int64_t *start) {
    const int64_t s = min(max(offsets[b], (int64_t)0), total), e = min(max(offsets[b + 1], (int64_t)0), total);
    *start = s;
    return max(e - s, (int64_t)0);
}

__device__ __forceinline__ float3 load_point(const FilterArgs &A, int64_t i) {
    const float *p = (const float *)(A.pts + (size_t)i * A.stride);
    return make_float3(p[0], p[1], p[2]);
}

// One workgroup: tbase = exclusive scan of the frames' tile counts, clamped at NT (reached only when offsets break their contract: a frame
// then has fewer tiles than points to fill them, and nothing out of bounds); kept and stats start at 0.
__global__ __launch_bounds__(256) void frames_kernel(const int64_t *__restrict__ offsets, int64_t total, int B, int NT, int32_t *__restrict__ tbase,
                                                     unsigned long long *__restrict__ kept, unsigned long long *__restrict__ stats) {
    __shared__ int s_v[256];
    int base = 0;
    for (int b0 = 0; b0 < B; b0 += 256) {
        const int b = b0 + threadIdx.x;
        int v = 0;
        if (b < B) {
            int64_t s;
            v = (int)((frame_range(offsets, b, total, &s) + FT - 1) / FT);   // <= 2^22
            if (kept) kept[b] = 0ull;
            if (stats) stats[2 * b] = 0ull, stats[2 * b + 1] = 0ull;
        }
        s_v[threadIdx.x] = v;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {   // Hillis-Steele inclusive scan (256 * 2^22 fits an int)
            const int a = threadIdx.x >= o ? s_v[threadIdx.x - o] : 0;
            __syncthreads();
            s_v[threadIdx.x] += a;
            __syncthreads();
        }
        if (b < B) tbase[b] = min(base + s_v[threadIdx.x] - v, NT);
        base = min(base + s_v[255], NT);
        __syncthreads();
    }
    if (threadIdx.x == 0) tbase[B] = base;
}

// The frame of tile t: the last b with tbase[b] <= t (empty frames repeat a value; the last of them owns the tile).  -1: not in use.
__device__ __forceinline__ int frame_of_tile(const int32_t *tbase, int B, int t) {
    if (t >= tbase[B]) return -1;
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tbase[mid] <= t) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// The points of tile t of frame b: [*start, *start + n), n in 0 .. 256.
__device__ __forceinline__ int tile_range(const FilterArgs &A, int b, int t, int64_t *start) {
    int64_t fs;
    const int64_t fn = frame_range(A.offsets, b, A.total, &fs);
    const int64_t o = (int64_t)(t - A.tbase[b]) * FT;
    *start = fs + o;
    return (int)min(max(fn - o, (int64_t)0), (int64_t)FT);
}

// Per tile: its frame, the box of its finite points and their count (a non-finite point must not poison the box: it is left out).
__global__ __launch_bounds__(256) void box_kernel(FilterArgs A, int32_t *__restrict__ tframe, float4 *__restrict__ boxes) {
    const int t = blockIdx.x;
    const int b = frame_of_tile(A.tbase, A.B, t);
    if (b < 0) {
        if (threadIdx.x == 0) tframe[t] = -1;
        return;
    }
    int64_t start;
    const int n = tile_range(A, b, t, &start);
    float3 p = make_float3(0.f, 0.f, 0.f);
    bool v = false;
    if ((int)threadIdx.x < n) {
        p = load_point(A, start + threadIdx.x);
        v = finite3(p.x, p.y, p.z);
    }
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
        tframe[t] = b;
        boxes[2 * (size_t)t] = make_float4(lx, ly, lz, __int_as_float(sc[0] + sc[1] + sc[2] + sc[3]));
        boxes[2 * (size_t)t + 1] = make_float4(hx, hy, hz, 0.f);
    }
}

// ------------------------------------------------------------------------------------------------
// search
// ------------------------------------------------------------------------------------------------
struct FilterParams {
    int nb_points;
    float lo, hi;   // screen bounds (see screen_nb)
    double r2;
};

struct FilterOut {
    uint8_t *keep;
    int32_t *count;
    unsigned long long *kept, *stats;
    char *masked;
};

template <bool BRUTE>
__global__ __launch_bounds__(256) void search_kernel(FilterArgs A, FilterParams prm, FilterOut O) {
    const int t0 = blockIdx.x, tid = threadIdx.x;
    const int b = A.tframe[t0];
    if (b < 0) return;   // a tile the batch does not use (uniform over the block)
    const int tb0 = A.tbase[b], Tf = A.tbase[b + 1] - tb0;   // the frame's tiles: tb0 .. tb0 + Tf - 1
    int64_t q0;
    const int qn = tile_range(A, b, t0, &q0);
    float3 q = make_float3(0.f, 0.f, 0.f);
    bool act = false;
    if (tid < qn) {
        q = load_point(A, q0 + tid);
        act = finite3(q.x, q.y, q.z);
    }
    const int need = prm.nb_points + 1;   // a lane stops counting here
    int cnt = 0;
    unsigned long long npair = 0, ntile = 0;

    __shared__ float4 s_pts[FT];                      // the staged tile: x, y, z, tag (< 0: no candidate)
    __shared__ int s_list[RPCC_FILTER_TILE_LIST];     // the round's candidate tiles
    __shared__ float s_box[4][6];
    __shared__ int s_w[4];

    // pending: the lane still needs candidates (brute force never stops early)
    auto pending = [&]() { return act && (BRUTE || cnt < need); };
    auto nb = [&](float x, float y, float z) {
        return BRUTE ? exact_nb(q.x, q.y, q.z, x, y, z, prm.r2) : screen_nb(q.x, q.y, q.z, x, y, z, prm.lo, prm.hi, prm.r2);
    };

    // Whether this lane has to look into tile t: it still needs candidates, and the tile's box does not prove that every pair fails (a bound
    // above the screen's hi).
    auto wants = [&](int t) {
        if (!pending()) return false;
        if (BRUTE) return true;
        const float4 lo = A.boxes[2 * (size_t)t], hi = A.boxes[2 * (size_t)t + 1];
        return box_bound(q, q, lo, hi) <= prm.hi;
    };

    auto scan_tile = [&](int t, bool use) {
        __syncthreads();   // the previous tile's readers are done
        int64_t c0;
        const int cn = tile_range(A, b, t, &c0);
        float4 v = make_float4(0.f, 0.f, 0.f, __int_as_float(-1));
        if (tid < cn) {
            const float3 p = load_point(A, c0 + tid);
            if (finite3(p.x, p.y, p.z)) v = make_float4(p.x, p.y, p.z, __int_as_float(0));
        }
        s_pts[tid] = v;
        __syncthreads();
        if (!use) return;
        ++ntile;
        // Eight candidates per step (the slots past cn carry tag < 0): their LDS reads are in flight together, and the lane looks at its
        // count once per step.  It may pass `need` inside a step; the count is clipped when it is written.
        for (int k = 0; k < cn; k += 8) {
            float4 c[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) c[j] = s_pts[k + j];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const bool valid = __float_as_int(c[j].w) >= 0;
                npair += valid ? 1 : 0;
                cnt += valid && nb(c[j].x, c[j].y, c[j].z) ? 1 : 0;
            }
            if (!BRUTE && cnt >= need) break;
        }
    };

    scan_tile(t0, act);   // the tile itself first (the point itself counts): a stored sweep's points usually stop here

    // The box of the lanes that still need candidates (all lanes of the tile under brute force, where it is not used).
    float3 qlo, qhi;
    {
        const bool p = pending();
        float lx = p ? q.x : INFINITY, ly = p ? q.y : INFINITY, lz = p ? q.z : INFINITY;
        float hx = p ? q.x : -INFINITY, hy = p ? q.y : -INFINITY, hz = p ? q.z : -INFINITY;
        lx = wave_min(lx), ly = wave_min(ly), lz = wave_min(lz);
        hx = wave_max(hx), hy = wave_max(hy), hz = wave_max(hz);
        const int w = tid >> 6;
        if ((tid & 63) == 0) s_box[w][0] = lx, s_box[w][1] = ly, s_box[w][2] = lz, s_box[w][3] = hx, s_box[w][4] = hy, s_box[w][5] = hz;
        __syncthreads();
        qlo = make_float3(fminf(fminf(s_box[0][0], s_box[1][0]), fminf(s_box[2][0], s_box[3][0])),
                          fminf(fminf(s_box[0][1], s_box[1][1]), fminf(s_box[2][1], s_box[3][1])),
                          fminf(fminf(s_box[0][2], s_box[1][2]), fminf(s_box[2][2], s_box[3][2])));
        qhi = make_float3(fmaxf(fmaxf(s_box[0][3], s_box[1][3]), fmaxf(s_box[2][3], s_box[3][3])),
                          fmaxf(fmaxf(s_box[0][4], s_box[1][4]), fmaxf(s_box[2][4], s_box[3][4])),
                          fmaxf(fmaxf(s_box[0][5], s_box[1][5]), fmaxf(s_box[2][5], s_box[3][5])));
    }

    for (int c0 = 0; c0 < Tf; c0 += RPCC_FILTER_TILE_LIST) {
        if (!__syncthreads_or(pending())) break;   // no lane needs more (uniform); also: every lane has read the previous round's list
        const int t = tb0 + c0 + tid;
        bool take = c0 + tid < Tf && t != t0;
        if (take && !BRUTE) {
            const float4 lo = A.boxes[2 * (size_t)t], hi = A.boxes[2 * (size_t)t + 1];
            take = __float_as_int(lo.w) > 0 && box_bound(qlo, qhi, lo, hi) <= prm.hi;
        }
        int nl;
        const int off = block_scan_flag(take, s_w, &nl);   // in tile order
        if (take) s_list[off] = t;
        __syncthreads();
        for (int i = 0; i < nl; ++i) {
            const int tc = s_list[i];
            const bool use = wants(tc);
            if (!BRUTE) {
                if ((i & 7) == 0 && !__syncthreads_or(pending())) break;   // the whole block is done (looked at every 8th tile)
                if (!__syncthreads_or(use)) continue;                      // the list is filtered by the box of all pending lanes: no single lane needs this tile
            }
            scan_tile(tc, use);
        }
    }

    const bool kp = act && cnt >= need;
    if (tid < qn) {
        const int64_t i = q0 + tid;
        O.keep[i] = kp ? 1 : 0;
        if (O.count) O.count[i] = act ? min(cnt, need) : 0;
        if (O.masked) {
            float *m = (float *)(O.masked + (size_t)i * A.stride);
            const float nan = __int_as_float(0x7fc00000);
            m[0] = kp ? q.x : nan, m[1] = kp ? q.y : nan, m[2] = kp ? q.z : nan;
            if (A.stride == 16) ((uint32_t *)m)[3] = ((const uint32_t *)(A.pts + (size_t)i * A.stride))[3];   // intensity: never interpreted
        }
    }
    const unsigned long long nk = __popcll(__ballot(kp));
    if (O.stats)
        for (int o = 32; o > 0; o >>= 1) npair += __shfl_xor(npair, o), ntile += __shfl_xor(ntile, o);
    if ((tid & 63) == 0) {
        if (O.kept && nk) atomicAdd(O.kept + b, nk);
        if (O.stats) {
            atomicAdd(O.stats + (size_t)b * RPCC_FILTER_NSTATS, npair);
            atomicAdd(O.stats + (size_t)b * RPCC_FILTER_NSTATS + 1, ntile);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
// The work buffer, carved here and nowhere else: [ boxes float4 [NT,2] | tframe int32 [NT] | tbase int32 [B+1] ], every part rounded up to
// 256 bytes, NT = total / 256 + B tiles (sum over the frames of ceil(n_b / 256) <= total / 256 + B).
struct Layout {
    int NT;
    size_t off_boxes, off_tframe, off_tbase, total;
};

static bool batch_ok(int64_t total, int B) { return B > 0 && B <= RPCC_FILTER_MAX_BATCH && total >= 0 && total <= RPCC_FILTER_MAX_POINTS; }

static Layout layout(int64_t total, int B) {
    Layout L;
    L.NT = (int)(total / FT) + B;
    size_t o = 0;
    L.off_boxes = o, o += al((size_t)L.NT * 2 * sizeof(float4));
    L.off_tframe = o, o += al((size_t)L.NT * 4);
    L.off_tbase = o, o += al((size_t)(B + 1) * 4);
    L.total = o;
    return L;
}

extern "C" size_t rpcc_filter_workspace_bytes(int64_t total, int B) { return batch_ok(total, B) ? layout(total, B).total : 0; }

extern "C" int rpcc_filter_radius(const float *points, int point_stride_bytes, const int64_t *offsets, int64_t total, int B, double radius,
                                  int nb_points, int flags, uint8_t *keep, int32_t *count, int64_t *kept, float *masked, int64_t *stats,
                                  void *ws, void *stream) {
    ARG_TRY(batch_ok(total, B));
    ARG_TRY(point_stride_bytes == 0 || point_stride_bytes == 12 || point_stride_bytes == 16);
    ARG_TRY(offsets && ws);
    ARG_TRY(total == 0 || (points && keep));
    ARG_TRY(masked == NULL || masked != points);
    ARG_TRY(radius > 0.0 && radius * radius >= 1e-30 && radius * radius <= 1e30);   // the screen's error bound (screen_nb); also rejects NaN
    ARG_TRY(nb_points >= 0 && nb_points < 0x7fffffff);
    ARG_TRY((flags & ~RPCC_FILTER_BRUTEFORCE) == 0);
    const Layout L = layout(total, B);
    hipStream_t st = (hipStream_t)stream;
    char *w = (char *)ws;
    float4 *boxes = (float4 *)(w + L.off_boxes);
    int32_t *tframe = (int32_t *)(w + L.off_tframe), *tbase = (int32_t *)(w + L.off_tbase);

    FilterArgs A;
    A.pts = (const char *)points, A.stride = point_stride_bytes == 16 ? 16 : 12;
    A.offsets = offsets, A.total = total, A.B = B;
    A.tbase = tbase, A.tframe = tframe, A.boxes = boxes;

    // screen_bounds: r^2 (1 -+ 8u), u = 2^-24, rounded inwards to fp32 (the same bounds as rpcc_seg_dbscan's)
    FilterParams prm;
    prm.nb_points = nb_points;
    prm.r2 = radius * radius;
    const double u8 = 8.0 * ldexp(1.0, -24), lo = prm.r2 * (1.0 - u8), hi = prm.r2 * (1.0 + u8);
    prm.lo = (float)lo;
    if ((double)prm.lo > lo) prm.lo = nextafterf(prm.lo, 0.f);
    prm.hi = (float)hi;
    if ((double)prm.hi < hi) prm.hi = nextafterf(prm.hi, INFINITY);

    FilterOut O;
    O.keep = keep, O.count = count, O.kept = (unsigned long long *)kept, O.stats = (unsigned long long *)stats, O.masked = (char *)masked;

    frames_kernel<<<1, 256, 0, st>>>(offsets, total, B, L.NT, tbase, O.kept, O.stats);
    box_kernel<<<L.NT, 256, 0, st>>>(A, tframe, boxes);
    if (flags & RPCC_FILTER_BRUTEFORCE) search_kernel<true><<<L.NT, 256, 0, st>>>(A, prm, O);
    else search_kernel<false><<<L.NT, 256, 0, st>>>(A, prm, O);
    LAUNCH_CHECK();
    return 0;
}
