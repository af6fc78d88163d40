// dbscan_kernels.hip -- librpcc_seg.so: DBSCAN segmentation (include/rpcc_seg.h) for gfx950.
//
// Per call, four small kernels prepare the frames (row_count, row_scan, rank, tile_box): the non-ground mask in fp64, the
// rank of every non-ground pixel in row-major order, its fp32 point, and per 8x32-pixel tile the bounding box of its real
// (non-zero-range) points.  The zero-range non-ground pixels are exact duplicates at the origin: they are one point of
// multiplicity Z, represented by the lowest of their ranks (o0), and their Z^2 pairs are never enumerated.
//
// search_kernel<MODE> then runs one workgroup of 256 threads per (query tile, frame), one query pixel per lane, over the
// tiles whose box can hold a neighbour:
//   CORE    counts neighbours (early exit at min_points) and writes the core flags (parent[r] = r, else -1);
//   UNION   hooks core-core edges into a union-find on ranks, the larger root onto the smaller (CAS), so that every
//           root is its component's lowest core rank;
//   BORDER  gives a non-core point the lowest cluster number among its core neighbours, pruned by a per-tile minimum.
// Between them: the origin point's core flag, root compression, and cluster numbers by an exclusive scan of the roots in
// rank order.  Components, roots and minima do not depend on the order anything is visited in, so pruned and brute-force
// results are equal bit for bit.
#include "../../include/rpcc_seg.h"
#include "../csrc_tile/tiles.h"

static_assert(RPCC_SEG_ERR_ARG == TILE_ERR_ARG && RPCC_SEG_ERR_HIP == TILE_ERR_HIP && RPCC_SEG_MAX_BATCH == TILE_MAX_BATCH &&
                  RPCC_SEG_MAX_PIXELS == TILE_MAX_PIXELS,
              "rpcc_seg.h and tiles.h disagree");

#define SG_CHUNK 4096  // ranks per workgroup of the cluster numbering (16 steps of 256)
#define SG_NFR 8       // ints per frame: n, Z, o0, real points near the origin, clusters, capped, origin core, spare

enum { FR_N = 0, FR_Z, FR_O0, FR_ONEAR, FR_NCL, FR_CAP, FR_OCORE };
enum { MODE_CORE = 0, MODE_UNION = 1, MODE_BORDER = 2 };

extern "C" int rpcc_seg_version(void) { return RPCC_SEG_ABI_VERSION; }
extern "C" const char *rpcc_seg_last_error(void) { return g_err; }

// ------------------------------------------------------------------------------------------------
// the neighbour test
// ------------------------------------------------------------------------------------------------
// Exact rule: ((dx*dx) + (dy*dy)) + (dz*dz) < eps*eps in fp64, un-fused, dx = double(xp) - double(xq).
__device__ __forceinline__ bool exact_nb(float px, float py, float pz, float qx, float qy, float qz, double e2) {
    const double dx = (double)px - (double)qx, dy = (double)py - (double)qy, dz = (double)pz - (double)qz;
    return ((dx * dx) + (dy * dy)) + (dz * dz) < e2;
}

// fp32 screen.  Let D be the exact (real-number) squared distance of the two fp32 points.  In fp32 a term dx*dx is
// (x_p - x_q)^2 (1+d1)^2 (1+d2) (the difference rounded once, the square once) and the two sums add at most two more
// factors, so d2f lies in D*[(1-u)^5, (1+u)^5], u = 2^-24; the fp64 evaluation lies in D*[(1-v)^5, (1+v)^5],
// v = 2^-53.  Hence d2f < eps^2 (1 - 8u) gives D < eps^2 (1 - 8u) / (1 - u)^5 < eps^2 (1 - 2.9u) and the fp64 value
// stays below eps^2: a neighbour.  d2f > eps^2 (1 + 8u) likewise gives an fp64 value above eps^2: not one.  lo / hi are
// those two bounds rounded inwards to fp32 on the host.  Underflow adds at most 15 * 2^-149 in absolute terms, negligible
// against eps^2 * 3u for eps^2 >= 1e-30 (checked by the entry); a d2f of +inf means D > FLT_MAX > eps^2; a NaN fails
// both comparisons and goes to the exact test.  Anything between lo and hi gets the exact test.
__device__ __forceinline__ bool screen_nb(float px, float py, float pz, float qx, float qy, float qz, float lo, float hi, double e2) {
    const float d = dist3(px, py, pz, qx, qy, qz);
    if (d < lo) return true;
    if (d > hi) return false;
    return exact_nb(px, py, pz, qx, qy, qz, e2);
}

// fp64 non-ground test: |double(r) - r_plane| > 0.5, r_plane = -d / ((a*A + b*B) + c*C); NaN is ground.
__device__ __forceinline__ bool nonground(float r, const float *t, const double *g) {
    const double den = ((double)t[0] * g[0] + (double)t[1] * g[1]) + (double)t[2] * g[2];
    const double res = (double)r - (-g[3] / den);
    return fabs(res) > 0.5;
}

// ------------------------------------------------------------------------------------------------
// union-find on ranks.  parent[r] <= r always (a root is hooked only onto a smaller root), so a find walks a strictly
// decreasing chain and ends within r + 1 steps; a failed CAS means the larger root was hooked meanwhile, so the next
// pair of roots has a strictly smaller sum, and a union ends within 2n retries.  Both loops carry those caps all the
// same: hitting one sets the frame's flag (max_label = RPCC_SEG_CAPPED) instead of spinning.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int ld_par(int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// HALVE: path halving (par[x] = its grandparent, still an ancestor) -- only while roots are being hooked; the
// compression pass must not use it, or a late halving store could overwrite a node's final root with an ancestor.
template <bool HALVE>
__device__ int find_root(int *par, int x, int cap, int *capped) {
    for (int i = 0; i < cap; ++i) {
        const int p = ld_par(par + x);
        if (p == x) return x;
        if (HALVE) {
            const int g = ld_par(par + p);
            if (g != p) __hip_atomic_store(par + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            x = g;
        } else {
            x = p;
        }
    }
    atomicOr(capped, 1);
    return x;
}

__device__ void unite(int *par, int a, int b, int cap, int *capped) {
    for (int it = 0; it < 2 * cap + 64; ++it) {
        a = find_root<true>(par, a, cap, capped);
        b = find_root<true>(par, b, cap, capped);
        if (a == b) return;
        const int hi = max(a, b), lo = min(a, b);
        const int old = atomicCAS(par + hi, hi, lo);
        if (old == hi) return;
        if (a == hi) a = old; else b = old;
    }
    atomicOr(capped, 1);
}

// ------------------------------------------------------------------------------------------------
// preparation
// ------------------------------------------------------------------------------------------------
__global__ void init_kernel(int32_t *__restrict__ frame, int32_t *__restrict__ max_label, unsigned long long *__restrict__ stats) {
    const int b = blockIdx.x, k = threadIdx.x;
    if (k < SG_NFR) frame[b * SG_NFR + k] = k == FR_O0 ? 0x7fffffff : 0;
    if (k == 0) max_label[b] = 0;
    if (stats && k < RPCC_SEG_NSTATS) stats[b * RPCC_SEG_NSTATS + k] = 0ull;
}

// row_count_kernel's predicate: a non-ground pixel.
struct IsNonground {
    const float *ri, *tm;
    const double *ground;
    __device__ bool operator()(int b, int h, int x, int H, int W) const {
        return nonground(ri[((size_t)b * H + h) * W + x], tm + ((size_t)h * W + x) * 3, ground + 4 * b);
    }
};

// pts[b][p] = (x, y, z, tag): tag = rank of a real point, -1 ground, -2 zero-range non-ground (the origin point).
__global__ __launch_bounds__(256) void rank_kernel(const float *__restrict__ ri, const float *__restrict__ tm,
                                                   const double *__restrict__ ground, int H, int W, const int32_t *__restrict__ rowoff,
                                                   float4 *__restrict__ pts, int32_t *__restrict__ frame) {
    const int h = blockIdx.x, b = blockIdx.y;
    const size_t P = (size_t)H * W;
    const float *row = ri + ((size_t)b * H + h) * W;
    const double *g = ground + 4 * b;
    __shared__ int s_w[4];
    int base = rowoff[(size_t)b * H + h];
    int nz = 0, zmin = 0x7fffffff;
    for (int x0 = 0; x0 < W; x0 += 256) {
        const int x = x0 + threadIdx.x;
        float r = 0.f;
        const float *t = tm + ((size_t)h * W + (x < W ? x : 0)) * 3;
        bool ng = false;
        if (x < W) {
            r = row[x];
            ng = nonground(r, t, g);
        }
        int tot;
        const int off = block_scan_flag(ng, s_w, &tot);
        if (x < W) {
            float4 v = make_float4(0.f, 0.f, 0.f, __int_as_float(-1));
            if (ng && r == 0.f) {
                v.w = __int_as_float(-2);
                ++nz;
                zmin = min(zmin, base + off);
            } else if (ng) {
                v = make_float4(r * t[0], r * t[1], r * t[2], __int_as_float(base + off));   // ops.backproject's fp32 products
            }
            pts[(size_t)b * P + (size_t)h * W + x] = v;
        }
        base += tot;
    }
    if (nz) {
        atomicAdd(frame + b * SG_NFR + FR_Z, nz);
        atomicMin(frame + b * SG_NFR + FR_O0, zmin);
    }
}

// tile_box_kernel's loader: the real points of pts (tag >= 0).
struct LoadReal {
    const float4 *pts;
    __device__ bool operator()(size_t i, float3 &p) const {
        const float4 q = pts[i];
        p = make_float3(q.x, q.y, q.z);
        return __float_as_int(q.w) >= 0;
    }
};

// ------------------------------------------------------------------------------------------------
// search
// ------------------------------------------------------------------------------------------------
struct SegWs {
    const float4 *pts;  // [B,P]
    const float4 *tiles;  // [B,T,2]
    const int32_t *tmin;  // [B,T] lowest cluster number among a tile's core points (INT_MAX: none)
    int32_t *par;       // [B,P] by rank: union-find parent of a core point, -1 otherwise
    int32_t *cl;        // [B,P] by rank: cluster number, -1 noise
    int32_t *frame;     // [B,SG_NFR]
};

struct SegParams {
    int H, W, ntc, T, brute, min_points;
    float lo, hi;   // screen bounds (see screen_nb)
    double e2;
};

template <int MODE>
__global__ __launch_bounds__(256) void search_kernel(SegWs S, SegParams prm, unsigned long long *stats) {
    const int t0 = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int H = prm.H, W = prm.W, ntc = prm.ntc, T = prm.T;
    const size_t P = (size_t)H * W, fb = (size_t)b * P;
    const float4 *tab = S.tiles + (size_t)b * T * 2;
    const float4 qlo4 = tab[2 * t0], qhi4 = tab[2 * t0 + 1];
    if (__float_as_int(qlo4.w) == 0) return;   // no real point in this tile (uniform over the block)
    int32_t *fr = S.frame + b * SG_NFR;
    const int n = fr[FR_N], Z = fr[FR_Z], o0 = fr[FR_O0];
    const bool ocore = fr[FR_OCORE] != 0;
    const int row = (t0 / ntc) * TILE_R + (tid >> 5), col = (t0 % ntc) * TILE_C + (tid & 31);
    float4 q = make_float4(0.f, 0.f, 0.f, __int_as_float(-1));
    if (row < H && col < W) q = S.pts[fb + (size_t)row * W + col];
    const int qr = __float_as_int(q.w);
    const bool brute = prm.brute != 0;
    auto nb = [&](float x, float y, float z) {
        return brute ? exact_nb(q.x, q.y, q.z, x, y, z, prm.e2) : screen_nb(q.x, q.y, q.z, x, y, z, prm.lo, prm.hi, prm.e2);
    };
    bool act = qr >= 0;
    const bool near_o = act && Z > 0 && nb(0.f, 0.f, 0.f);
    int cnt = 0, best = 0x7fffffff;
    if (MODE == MODE_CORE) {
        if (near_o) {
            cnt = Z;
            atomicAdd(fr + FR_ONEAR, 1);
        }
    } else if (MODE == MODE_UNION) {
        act = act && S.par[fb + qr] >= 0;
        if (act && ocore && near_o) unite(S.par + fb, qr, o0, n + 1, fr + FR_CAP);
    } else {
        act = act && S.par[fb + qr] < 0;
        if (act && ocore && near_o) best = S.cl[fb + o0];
    }
    unsigned long long npair = 0, ntile = 0;

    __shared__ float4 s_pts[256];
    __shared__ int s_list[TILE_LIST];
    __shared__ int s_cnt, s_maxb;

    // pending: the lane still needs candidates (CORE: fewer than min_points found so far; brute force never stops early)
    auto pending = [&]() { return act && (MODE != MODE_CORE || brute || cnt < prm.min_points); };

    auto scan_tile = [&](int t) {
        __syncthreads();   // the previous tile's readers are done
        const int sr = (t / ntc) * TILE_R + (tid >> 5), sc = (t % ntc) * TILE_C + (tid & 31);
        float4 v = make_float4(0.f, 0.f, 0.f, __int_as_float(-1));   // tag < 0: no candidate
        if (sr < H && sc < W) {
            const float4 p = S.pts[fb + (size_t)sr * W + sc];
            const int r = __float_as_int(p.w);
            if (r >= 0) {
                if (MODE == MODE_CORE) v = p;
                else if (S.par[fb + r] >= 0) v = make_float4(p.x, p.y, p.z, __int_as_float(MODE == MODE_UNION ? r : S.cl[fb + r]));
            }
        }
        s_pts[tid] = v;
        __syncthreads();
        if (!pending()) return;
        if (!brute) {
            const float4 lo = tab[2 * t], hi = tab[2 * t + 1];   // a bound above the screen's hi: every pair of the tile fails
            if (box_bound(make_float3(q.x, q.y, q.z), make_float3(q.x, q.y, q.z), lo, hi) > prm.hi) return;
            if (MODE == MODE_BORDER && S.tmin[(size_t)b * T + t] >= best) return;
        }
        ++ntile;
        for (int k = 0; k < 256; ++k) {
            const float4 c = s_pts[k];
            const int tag = __float_as_int(c.w);
            if (tag < 0) continue;
            if (MODE == MODE_UNION && tag >= qr) continue;   // each core-core edge once, from its higher rank
            ++npair;
            if (!nb(c.x, c.y, c.z)) continue;
            if (MODE == MODE_CORE) {
                if (++cnt >= prm.min_points && !brute) break;
            } else if (MODE == MODE_UNION) {
                unite(S.par + fb, qr, tag, n + 1, fr + FR_CAP);
            } else {
                best = min(best, tag);
            }
        }
    };

    scan_tile(t0);   // the co-located tile first: CORE usually stops there
    const float3 qlo = make_float3(qlo4.x, qlo4.y, qlo4.z), qhi = make_float3(qhi4.x, qhi4.y, qhi4.z);
    for (int c0 = 0; c0 < T; c0 += TILE_LIST) {
        __syncthreads();   // every lane has read s_cnt / s_list of the previous round
        if (tid == 0) s_cnt = 0, s_maxb = -1;
        __syncthreads();
        if (pending()) atomicMax(&s_maxb, MODE == MODE_BORDER ? best : 0);
        __syncthreads();
        const int maxb = s_maxb;
        if (maxb < 0) break;   // no lane needs more candidates (uniform: read after the barrier)
        const int c1 = min(T, c0 + TILE_LIST);
        for (int t = c0 + tid; t < c1; t += 256) {
            if (t == t0) continue;
            bool keep = brute;
            if (!keep) {
                const float4 lo = tab[2 * t], hi = tab[2 * t + 1];
                keep = __float_as_int(lo.w) > 0 && box_bound(qlo, qhi, lo, hi) <= prm.hi &&
                       (MODE != MODE_BORDER || S.tmin[(size_t)b * T + t] < maxb);
            }
            if (keep) s_list[atomicAdd(&s_cnt, 1)] = t;
        }
        __syncthreads();
        const int nl = s_cnt;
        for (int i = 0; i < nl; ++i) {
            if (MODE == MODE_CORE && !__syncthreads_or(pending())) break;   // the whole block is done
            scan_tile(s_list[i]);
        }
    }

    if (act) {
        if (MODE == MODE_CORE) S.par[fb + qr] = cnt >= prm.min_points ? qr : -1;
        if (MODE == MODE_BORDER) S.cl[fb + qr] = best == 0x7fffffff ? -1 : best;
    }
    if (stats) {
        for (int o = 32; o > 0; o >>= 1) npair += __shfl_xor(npair, o), ntile += __shfl_xor(ntile, o);
        if ((tid & 63) == 0) {
            atomicAdd(stats + (size_t)b * RPCC_SEG_NSTATS, npair);
            atomicAdd(stats + (size_t)b * RPCC_SEG_NSTATS + 1, ntile);
        }
    }
}

// The origin point: core when Z + (real points within eps of the origin) >= min_points.
__global__ void origin_kernel(int32_t *__restrict__ frame, int32_t *__restrict__ par, size_t P, int min_points) {
    const int b = blockIdx.x;
    int32_t *fr = frame + b * SG_NFR;
    const int Z = fr[FR_Z];
    if (threadIdx.x == 0 && Z > 0 && (long long)Z + fr[FR_ONEAR] >= min_points) {
        fr[FR_OCORE] = 1;
        par[(size_t)b * P + fr[FR_O0]] = fr[FR_O0];
    }
}

__global__ __launch_bounds__(256) void compress_kernel(int32_t *__restrict__ par, int32_t *__restrict__ frame, size_t P) {
    const int b = blockIdx.y;
    const int r = blockIdx.x * 256 + threadIdx.x;
    int32_t *fr = frame + b * SG_NFR;
    const int n = fr[FR_N];
    if (r >= n) return;
    int *pb = par + (size_t)b * P;
    if (ld_par(pb + r) < 0) return;
    const int root = find_root<false>(pb, r, n + 1, fr + FR_CAP);
    __hip_atomic_store(pb + r, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Roots (core ranks with par[r] == r) per chunk of SG_CHUNK ranks.
__global__ __launch_bounds__(256) void root_count_kernel(const int32_t *__restrict__ par, const int32_t *__restrict__ frame, size_t P,
                                                         int nch, int32_t *__restrict__ chcnt) {
    const int ch = blockIdx.x, b = blockIdx.y;
    const int n = frame[b * SG_NFR + FR_N];
    const int32_t *pb = par + (size_t)b * P;
    int c = 0;
    for (int r = ch * SG_CHUNK + threadIdx.x; r < min(n, (ch + 1) * SG_CHUNK); r += 256) c += pb[r] == r ? 1 : 0;
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    __shared__ int s[4];
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) chcnt[(size_t)b * nch + ch] = s[0] + s[1] + s[2] + s[3];
}

// cl[root] = cluster number: the exclusive count of roots of lower rank.
__global__ __launch_bounds__(256) void root_number_kernel(const int32_t *__restrict__ par, const int32_t *__restrict__ frame, size_t P,
                                                          int nch, const int32_t *__restrict__ choff, int32_t *__restrict__ cl) {
    const int ch = blockIdx.x, b = blockIdx.y;
    const int n = frame[b * SG_NFR + FR_N];
    const int32_t *pb = par + (size_t)b * P;
    __shared__ int s_w[4];
    int base = choff[(size_t)b * nch + ch];
    for (int r0 = ch * SG_CHUNK; r0 < (ch + 1) * SG_CHUNK; r0 += 256) {
        const int r = r0 + threadIdx.x;
        const bool f = r < n && pb[r] == r;
        int tot;
        const int off = block_scan_flag(f, s_w, &tot);
        if (f) cl[(size_t)b * P + r] = base + off;
        base += tot;
    }
}

// Core points take their root's number, the others -1 (BORDER fills in border points).
__global__ __launch_bounds__(256) void core_label_kernel(const int32_t *__restrict__ par, const int32_t *__restrict__ frame, size_t P,
                                                         int32_t *__restrict__ cl) {
    const int b = blockIdx.y;
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= frame[b * SG_NFR + FR_N]) return;
    const int p = par[(size_t)b * P + r];
    if (p != r) cl[(size_t)b * P + r] = p >= 0 ? cl[(size_t)b * P + p] : -1;   // a root keeps its number
}

// Per tile: the lowest cluster number of its core real points.
__global__ __launch_bounds__(256) void tile_min_kernel(const float4 *__restrict__ pts, const int32_t *__restrict__ par,
                                                       const int32_t *__restrict__ cl, int H, int W, int ntc, int T,
                                                       int32_t *__restrict__ tmin) {
    const int t = blockIdx.x, b = blockIdx.y;
    const size_t P = (size_t)H * W;
    const int row = (t / ntc) * TILE_R + (threadIdx.x >> 5), col = (t % ntc) * TILE_C + (threadIdx.x & 31);
    int m = 0x7fffffff;
    if (row < H && col < W) {
        const int r = __float_as_int(pts[(size_t)b * P + (size_t)row * W + col].w);
        if (r >= 0 && par[(size_t)b * P + r] >= 0) m = cl[(size_t)b * P + r];
    }
    for (int o = 32; o > 0; o >>= 1) m = min(m, __shfl_xor(m, o));
    __shared__ int s[4];
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) tmin[(size_t)b * T + t] = min(min(s[0], s[1]), min(s[2], s[3]));
}

// Final labels (segment_utils.py:161-169): ground 0, noise 2, cluster k -> k + 3, then every ri == 0 pixel 1.
__global__ __launch_bounds__(256) void label_kernel(const float *__restrict__ ri, const float4 *__restrict__ pts,
                                                    const int32_t *__restrict__ cl, size_t P, int32_t *__restrict__ seg,
                                                    int32_t *__restrict__ max_label) {
    const int b = blockIdx.y;
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    int lab = 0;
    if (p < P) {
        const int tag = __float_as_int(pts[(size_t)b * P + p].w);
        if (ri[(size_t)b * P + p] == 0.f) lab = 1;
        else if (tag >= 0) {
            const int c = cl[(size_t)b * P + tag];
            lab = c < 0 ? 2 : c + 3;
        }
        seg[(size_t)b * P + p] = lab;
    }
    for (int o = 32; o > 0; o >>= 1) lab = max(lab, __shfl_xor(lab, o));
    if ((threadIdx.x & 63) == 0 && lab > 0) atomicMax(max_label + b, lab);
}

__global__ void finish_kernel(const int32_t *__restrict__ frame, int32_t *__restrict__ max_label) {
    const int b = blockIdx.x;
    if (threadIdx.x == 0 && frame[b * SG_NFR + FR_CAP]) max_label[b] = RPCC_SEG_CAPPED;
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
struct Layout {
    int ntc, T, nch;
    size_t P, off_pts, off_tiles, off_tmin, off_par, off_cl, off_rowcnt, off_rowoff, off_chcnt, off_choff, off_frame, total;
};

static Layout layout(int B, int H, int W) {
    Layout L;
    L.P = (size_t)H * W;
    L.ntc = tile_cols(W);
    L.T = tile_count(H, W);
    L.nch = (int)((L.P + SG_CHUNK - 1) / SG_CHUNK);
    size_t o = 0;
    L.off_pts = o, o += al((size_t)B * L.P * sizeof(float4));
    L.off_tiles = o, o += al((size_t)B * L.T * 2 * sizeof(float4));
    L.off_tmin = o, o += al((size_t)B * L.T * 4);
    L.off_par = o, o += al((size_t)B * L.P * 4);
    L.off_cl = o, o += al((size_t)B * L.P * 4);
    L.off_rowcnt = o, o += al((size_t)B * H * 4);
    L.off_rowoff = o, o += al((size_t)B * H * 4);
    L.off_chcnt = o, o += al((size_t)B * L.nch * 4);
    L.off_choff = o, o += al((size_t)B * L.nch * 4);
    L.off_frame = o, o += al((size_t)B * SG_NFR * 4);
    L.total = o;
    return L;
}

extern "C" size_t rpcc_seg_workspace_bytes(int B, int H, int W) { return shape_ok(B, H, W) ? layout(B, H, W).total : 0; }

extern "C" int rpcc_seg_dbscan(const float *ri, const float *tm, const double *ground, int B, int H, int W, double eps, int min_points,
                               int flags, int32_t *seg, int32_t *max_label, int64_t *stats, void *ws, void *stream) {
    ARG_TRY(shape_ok(B, H, W));
    ARG_TRY(ri && tm && ground && seg && max_label && ws);
    ARG_TRY(eps > 0.0 && eps * eps >= 1e-30 && eps * eps <= 1e30);   // the screen's error bound (screen_nb); also rejects NaN
    ARG_TRY(min_points >= 1);
    ARG_TRY((flags & ~RPCC_SEG_BRUTEFORCE) == 0);
    const Layout L = layout(B, H, W);
    hipStream_t st = (hipStream_t)stream;
    char *w = (char *)ws;
    SegWs S;
    S.pts = (const float4 *)(w + L.off_pts);
    S.tiles = (const float4 *)(w + L.off_tiles);
    S.tmin = (const int32_t *)(w + L.off_tmin);
    S.par = (int32_t *)(w + L.off_par);
    S.cl = (int32_t *)(w + L.off_cl);
    S.frame = (int32_t *)(w + L.off_frame);
    int32_t *rowcnt = (int32_t *)(w + L.off_rowcnt), *rowoff = (int32_t *)(w + L.off_rowoff);
    int32_t *chcnt = (int32_t *)(w + L.off_chcnt), *choff = (int32_t *)(w + L.off_choff);
    unsigned long long *st64 = (unsigned long long *)stats;

    SegParams prm;
    prm.H = H, prm.W = W, prm.ntc = L.ntc, prm.T = L.T;
    prm.brute = flags & RPCC_SEG_BRUTEFORCE;
    prm.min_points = min_points;
    prm.e2 = eps * eps;
    const double u8 = 8.0 * ldexp(1.0, -24), lo = prm.e2 * (1.0 - u8), hi = prm.e2 * (1.0 + u8);
    prm.lo = (float)lo;
    if ((double)prm.lo > lo) prm.lo = nextafterf(prm.lo, 0.f);
    prm.hi = (float)hi;
    if ((double)prm.hi < hi) prm.hi = nextafterf(prm.hi, INFINITY);

    const unsigned pblocks = (unsigned)((L.P + 255) / 256);
    init_kernel<<<B, 64, 0, st>>>(S.frame, max_label, st64);
    HIP_TRY(hipMemsetAsync(S.par, 0xff, (size_t)B * L.P * 4, st));
    row_count_kernel<<<dim3(H, B), 256, 0, st>>>(IsNonground{ri, tm, ground}, H, W, rowcnt);
    scan_kernel<SG_NFR><<<B, 256, 0, st>>>(rowcnt, H, rowoff, S.frame + FR_N);
    rank_kernel<<<dim3(H, B), 256, 0, st>>>(ri, tm, ground, H, W, rowoff, (float4 *)S.pts, S.frame);
    tile_box_kernel<<<dim3(L.T, B), 256, 0, st>>>(LoadReal{S.pts}, H, W, L.ntc, L.T, (float4 *)S.tiles);
    search_kernel<MODE_CORE><<<dim3(L.T, B), 256, 0, st>>>(S, prm, st64);
    origin_kernel<<<B, 64, 0, st>>>(S.frame, S.par, L.P, min_points);
    search_kernel<MODE_UNION><<<dim3(L.T, B), 256, 0, st>>>(S, prm, st64);
    compress_kernel<<<dim3(pblocks, B), 256, 0, st>>>(S.par, S.frame, L.P);
    root_count_kernel<<<dim3(L.nch, B), 256, 0, st>>>(S.par, S.frame, L.P, L.nch, chcnt);
    scan_kernel<SG_NFR><<<B, 256, 0, st>>>(chcnt, L.nch, choff, S.frame + FR_NCL);
    root_number_kernel<<<dim3(L.nch, B), 256, 0, st>>>(S.par, S.frame, L.P, L.nch, choff, S.cl);
    core_label_kernel<<<dim3(pblocks, B), 256, 0, st>>>(S.par, S.frame, L.P, S.cl);
    tile_min_kernel<<<dim3(L.T, B), 256, 0, st>>>(S.pts, S.par, S.cl, H, W, L.ntc, L.T, (int32_t *)S.tmin);
    search_kernel<MODE_BORDER><<<dim3(L.T, B), 256, 0, st>>>(S, prm, st64);
    label_kernel<<<dim3(pblocks, B), 256, 0, st>>>(ri, S.pts, S.cl, L.P, seg, max_label);
    finish_kernel<<<B, 64, 0, st>>>(S.frame, max_label);
    LAUNCH_CHECK();
    return 0;
}
