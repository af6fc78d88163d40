// eval_kernels.hip -- librpcc_eval.so: reconstruction-quality metrics (include/rpcc_eval.h) for gfx950.
//
// Per call and cloud, four small kernels prepare the frame (tile_box, row_count, scan, rank): validity, the rank of
// every valid pixel in row-major order, the pixel of every rank, and per 8x32-pixel tile the bounding box of its valid
// points and their count.  search_kernel then runs one workgroup of 256 threads per (query tile, frame), one query per
// lane: exact nearest neighbour (NnState) or the 12 nearest within r (KnnState, followed by the fp64 covariance and its
// eigenvector).  The metrics entry carries cloud 1's normals over to cloud 2 with fixed-point atomics and reduces every
// per-point term of a frame in fp64 in a fixed order (partial sums per chunk, then one pass over the chunks).
#include "../../include/rpcc_eval.h"
#include "../csrc_tile/tiles.h"

static_assert(RPCC_EVAL_ERR_ARG == TILE_ERR_ARG && RPCC_EVAL_ERR_HIP == TILE_ERR_HIP && RPCC_EVAL_MAX_BATCH == TILE_MAX_BATCH &&
                  RPCC_EVAL_MAX_PIXELS == TILE_MAX_PIXELS,
              "rpcc_eval.h and tiles.h disagree");

#define EV_CHUNK 4096 // points per workgroup of the metrics reduction

extern "C" int rpcc_eval_version(void) { return RPCC_EVAL_ABI_VERSION; }
extern "C" const char *rpcc_eval_last_error(void) { return g_err; }

// ------------------------------------------------------------------------------------------------
// geometry helpers
// ------------------------------------------------------------------------------------------------
struct Cloud {
    const float *pts;  // [B,P,3]
    int32_t *rank;     // [B,P] rank of a valid pixel, -1 elsewhere
    int32_t *pix;      // [B,P] pixel of rank i (first n[b] entries)
    int32_t *rowcnt;   // [B,H] valid pixels per row
    int32_t *rowoff;   // [B,H] exclusive prefix of rowcnt
    int32_t *n;        // n[2*b]: valid points of frame b (the two clouds' counts interleave: rpcc_eval_nn's n layout)
    float4 *tiles;     // [B,T,2]: (lo.xyz, count as int bits), (hi.xyz, 0)
};

__device__ __forceinline__ bool valid3(float x, float y, float z) { return ((x + y) + z) != 0.f; }

// ------------------------------------------------------------------------------------------------
// preparation: tile boxes, row counts, row offsets, ranks
// ------------------------------------------------------------------------------------------------
// tile_box_kernel's loader and row_count_kernel's predicate: a pixel of the cloud f32 [B,H,W,3] that holds a point.
struct LoadPoint {
    const float *pts;
    __device__ bool operator()(size_t i, float3 &p) const {
        const float *q = pts + i * 3;
        p = make_float3(q[0], q[1], q[2]);
        return valid3(p.x, p.y, p.z);
    }
};
struct IsPoint {
    const float *pts;
    __device__ bool operator()(int b, int h, int x, int H, int W) const {
        const float *row = pts + ((size_t)b * H + h) * (size_t)W * 3;
        return valid3(row[3 * x], row[3 * x + 1], row[3 * x + 2]);
    }
};

__global__ __launch_bounds__(256) void rank_kernel(const float *__restrict__ pts, int H, int W, const int32_t *__restrict__ rowoff,
                                                   int32_t *__restrict__ rank, int32_t *__restrict__ pix) {
    const int h = blockIdx.x, b = blockIdx.y;
    const size_t P = (size_t)H * W;
    const float *row = pts + ((size_t)b * P + (size_t)h * W) * 3;
    __shared__ int s_w[4];
    int base = rowoff[(size_t)b * H + h];
    for (int x0 = 0; x0 < W; x0 += 256) {
        const int x = x0 + threadIdx.x;
        const bool v = x < W && valid3(row[3 * x], row[3 * x + 1], row[3 * x + 2]);
        int tot;
        const int off = block_scan_flag(v, s_w, &tot);
        if (x < W) {
            const int p = h * W + x;
            rank[(size_t)b * P + p] = v ? base + off : -1;
            if (v) pix[(size_t)b * P + base + off] = p;
        }
        base += tot;
    }
}

// ------------------------------------------------------------------------------------------------
// search: exact nearest neighbour / 12 nearest within r, tile-pruned
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool before(float d, int p, float bd, int bp) { return d < bd || (d == bd && p < bp); }

struct NnState {
    float best;
    int bi;  // pixel of the best point; INT_MAX = none yet
    __device__ void init(float) { best = INFINITY, bi = 0x7fffffff; }
    __device__ float bound() const { return best; }
    __device__ __forceinline__ void consider(float d, int p) {
        if (before(d, p, best, bi)) best = d, bi = p;
    }
};

struct KnnState {
    float kd[RPCC_EVAL_KNN];
    int ki[RPCC_EVAL_KNN];
    float r2;
    __device__ void init(float r2_) {
        r2 = r2_;
#pragma unroll
        for (int k = 0; k < RPCC_EVAL_KNN; ++k) kd[k] = INFINITY, ki[k] = 0x7fffffff;
    }
    // A candidate counts only with d <= r2; once 12 are held it must also precede the 12th.
    __device__ float bound() const { return fminf(kd[RPCC_EVAL_KNN - 1], r2); }
    __device__ __forceinline__ void consider(float d, int p) {
        if (!(d <= r2) || !before(d, p, kd[RPCC_EVAL_KNN - 1], ki[RPCC_EVAL_KNN - 1])) return;
        bool placed = false;
#pragma unroll
        for (int k = RPCC_EVAL_KNN - 1; k >= 0; --k) {   // sorted insertion, fully unrolled: the list stays in registers
            if (!placed) {
                if (k > 0 && before(d, p, kd[k - 1], ki[k - 1])) {
                    kd[k] = kd[k - 1], ki[k] = ki[k - 1];
                } else {
                    kd[k] = d, ki[k] = p;
                    placed = true;
                }
            }
        }
    }
};

// Jacobi rotation of the symmetric 3x3 matrix (diagonal a*, off-diagonal o*) in the (p, q) plane; r is the third index.
#define EV_ROT(app, aqq, apq, arp, arq, P_, Q_)                                                 \
    if (apq != 0.0) {                                                                            \
        const double th = (aqq - app) / (2.0 * apq);                                             \
        const double t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));           \
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;                                     \
        app -= t * apq;                                                                          \
        aqq += t * apq;                                                                          \
        apq = 0.0;                                                                               \
        const double rp = c * arp - s * arq, rq = s * arp + c * arq;                             \
        arp = rp, arq = rq;                                                                      \
        for (int k_ = 0; k_ < 3; ++k_) {                                                         \
            const double vp = v[k_][P_], vq = v[k_][Q_];                                         \
            v[k_][P_] = c * vp - s * vq, v[k_][Q_] = s * vp + c * vq;                            \
        }                                                                                        \
    }

// Unit eigenvector of the smallest eigenvalue of [[a0 o01 o02] [o01 a1 o12] [o02 o12 a2]] (cyclic Jacobi, fp64).
__device__ void min_eigvec(double a0, double a1, double a2, double o01, double o02, double o12, double *n) {
    double v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    const double scale = fabs(a0) + fabs(a1) + fabs(a2) + fabs(o01) + fabs(o02) + fabs(o12);
#pragma unroll 1
    for (int sweep = 0; sweep < 12; ++sweep) {
        if (fabs(o01) + fabs(o02) + fabs(o12) <= 1e-18 * scale) break;
        EV_ROT(a0, a1, o01, o02, o12, 0, 1)
        EV_ROT(a0, a2, o02, o01, o12, 0, 2)
        EV_ROT(a1, a2, o12, o01, o02, 1, 2)
    }
    const int m = (a0 <= a1 && a0 <= a2) ? 0 : (a1 <= a2 ? 1 : 2);
    double x = m == 0 ? v[0][0] : m == 1 ? v[0][1] : v[0][2];
    double y = m == 0 ? v[1][0] : m == 1 ? v[1][1] : v[1][2];
    double z = m == 0 ? v[2][0] : m == 1 ? v[2][1] : v[2][2];
    const double inv = 1.0 / sqrt(x * x + y * y + z * z);
    n[0] = x * inv, n[1] = y * inv, n[2] = z * inv;
}

struct NnOut {
    float *dist;
    int32_t *idx;
};
struct KnnOut {
    double *normals;
    int32_t *nbr;
};

__device__ __forceinline__ void finish(const NnState &st, const NnOut &o, const Cloud &S, size_t fb, int qrank, float, float, float,
                                       const float *) {
    o.dist[fb + qrank] = st.bi == 0x7fffffff ? NAN : st.best;
    o.idx[fb + qrank] = st.bi == 0x7fffffff ? -1 : S.rank[fb + st.bi];
}

__device__ __forceinline__ void finish(const KnnState &st, const KnnOut &o, const Cloud &S, size_t fb, int qrank, float qx, float qy,
                                       float qz, const float *spts) {
    int m = 0;
    double sx = 0.0, sy = 0.0, sz = 0.0;
#pragma unroll
    for (int k = 0; k < RPCC_EVAL_KNN; ++k) {
        if (st.ki[k] != 0x7fffffff) {
            const float *p = spts + 3 * (size_t)st.ki[k];
            sx += (double)p[0], sy += (double)p[1], sz += (double)p[2];
            ++m;
        }
        if (o.nbr) o.nbr[(fb + qrank) * RPCC_EVAL_KNN + k] = st.ki[k] != 0x7fffffff ? S.rank[fb + st.ki[k]] : -1;
    }
    double nrm[3] = {0.0, 0.0, 1.0};
    if (m >= 3) {   // two passes: the mean, then the centred second moments
        const double mx = sx / m, my = sy / m, mz = sz / m;
        double cxx = 0.0, cyy = 0.0, czz = 0.0, cxy = 0.0, cxz = 0.0, cyz = 0.0;
#pragma unroll
        for (int k = 0; k < RPCC_EVAL_KNN; ++k) {
            if (st.ki[k] != 0x7fffffff) {
                const float *p = spts + 3 * (size_t)st.ki[k];
                const double dx = (double)p[0] - mx, dy = (double)p[1] - my, dz = (double)p[2] - mz;
                cxx += dx * dx, cyy += dy * dy, czz += dz * dz, cxy += dx * dy, cxz += dx * dz, cyz += dy * dz;
            }
        }
        min_eigvec(cxx / m, cyy / m, czz / m, cxy / m, cxz / m, cyz / m, nrm);
        if (nrm[0] * (double)qx + nrm[1] * (double)qy + nrm[2] * (double)qz > 0.0) nrm[0] = -nrm[0], nrm[1] = -nrm[1], nrm[2] = -nrm[2];
    }
    double *o3 = o.normals + (fb + qrank) * 3;
    o3[0] = nrm[0], o3[1] = nrm[1], o3[2] = nrm[2];
}

__device__ __forceinline__ void empty_target(const NnOut &o, size_t fb, int qrank) {
    o.dist[fb + qrank] = NAN;
    o.idx[fb + qrank] = -1;
}
__device__ __forceinline__ void empty_target(const KnnOut &, size_t, int) {}   // the query cloud itself: never empty here

// One workgroup per (query tile, frame); lane l holds the query pixel (row 8*tr + l/32, column 32*tc + l%32).
//   1. seed: the target tile at the same position (the clouds share pixels: usually the answer already);
//   2. rounds of up to TILE_LIST target tiles: keep those whose box bound to the query tile's box is <= the largest lane
//      bound, stage each kept tile's points in LDS, and let every lane whose own point-to-box bound is <= its bound scan them.
// A tile is skipped only when its box_bound > the bound, never at equality (a tile at equality may hold an equal distance with
// a lower rank).  Brute force: every tile, no bound.  The result is the minimum of (distance, pixel) over the scanned
// candidates, which does not depend on the order the tiles are visited in: pruned and brute force agree bit for bit.
template <class State, class Out>
__global__ __launch_bounds__(256) void search_kernel(Cloud Q, Cloud S, int H, int W, int ntc, int T, int brute, float r2, Out out,
                                                     int32_t *visits) {
    const int t0 = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const size_t P = (size_t)H * W, fb = (size_t)b * P;
    const float4 *qt = Q.tiles + ((size_t)b * T + t0) * 2;
    const float4 qlo4 = qt[0], qhi4 = qt[1];
    if (__float_as_int(qlo4.w) == 0) return;   // no query in this tile (uniform over the block)
    const float4 *stab = S.tiles + (size_t)b * T * 2;
    const float *spts = S.pts + fb * 3;
    const int row = (t0 / ntc) * TILE_R + (tid >> 5), col = (t0 % ntc) * TILE_C + (tid & 31);
    const bool in_img = row < H && col < W;
    const int qp = in_img ? row * W + col : 0;
    const int qrank = in_img ? Q.rank[fb + qp] : -1;
    const bool act = qrank >= 0;
    float qx = 0.f, qy = 0.f, qz = 0.f;
    if (act) {
        const float *q = Q.pts + (fb + qp) * 3;
        qx = q[0], qy = q[1], qz = q[2];
    }
    if (S.n[2 * b] == 0) {
        if (act) empty_target(out, fb, qrank);
        return;
    }
    State st;
    st.init(r2);
    int nvis = 0;

    __shared__ float4 s_pts[256];
    __shared__ int s_list[TILE_LIST];
    __shared__ int s_cnt;
    __shared__ unsigned s_maxb;

    auto scan_tile = [&](int t, bool check) {
        __syncthreads();   // the previous tile's readers are done
        const int sr = (t / ntc) * TILE_R + (tid >> 5), sc = (t % ntc) * TILE_C + (tid & 31);
        float4 v = make_float4(NAN, NAN, NAN, 0.f);   // no point: NaN coordinates, a distance no comparison accepts
        if (sr < H && sc < W) {
            const int sp = sr * W + sc;
            const float *p = spts + (size_t)sp * 3;
            const float x = p[0], y = p[1], z = p[2];
            if (valid3(x, y, z)) v = make_float4(x, y, z, __int_as_float(sp));
        }
        s_pts[tid] = v;
        __syncthreads();
        if (!act) return;
        if (check) {
            const float4 lo = stab[2 * t], hi = stab[2 * t + 1];
            if (box_bound(make_float3(qx, qy, qz), make_float3(qx, qy, qz), lo, hi) > st.bound()) return;
        }
        ++nvis;
#pragma unroll 8
        for (int k = 0; k < 256; ++k) {
            const float4 c = s_pts[k];
            st.consider(dist3(qx, qy, qz, c.x, c.y, c.z), __float_as_int(c.w));
        }
    };

    scan_tile(t0, false);
    const float3 qlo = make_float3(qlo4.x, qlo4.y, qlo4.z), qhi = make_float3(qhi4.x, qhi4.y, qhi4.z);
    for (int c0 = 0; c0 < T; c0 += TILE_LIST) {
        __syncthreads();   // every lane has read s_cnt / s_list of the previous round
        if (tid == 0) s_cnt = 0, s_maxb = 0u;
        __syncthreads();
        if (act) atomicMax(&s_maxb, __float_as_uint(st.bound()));   // bounds are >= 0 (or +inf): their bits order as unsigned
        __syncthreads();
        const float maxb = __uint_as_float(s_maxb);
        const int c1 = min(T, c0 + TILE_LIST);
        for (int t = c0 + tid; t < c1; t += 256) {
            if (t == t0) continue;
            bool keep = brute != 0;
            if (!keep) {
                const float4 lo = stab[2 * t], hi = stab[2 * t + 1];
                keep = __float_as_int(lo.w) > 0 && box_bound(qlo, qhi, lo, hi) <= maxb;
            }
            if (keep) s_list[atomicAdd(&s_cnt, 1)] = t;
        }
        __syncthreads();
        const int nl = s_cnt;
        for (int i = 0; i < nl; ++i) scan_tile(s_list[i], brute == 0);
    }
    if (!act) return;
    finish(st, out, S, fb, qrank, qx, qy, qz, spts);
    if (visits) visits[fb * 2 + qrank] = nvis + 1;   // + the seed tile (visits is [B,2,P]: fb*2 selects frame b)
}

// ------------------------------------------------------------------------------------------------
// metrics: normal transfer (assign_attr) and per-frame sums
// ------------------------------------------------------------------------------------------------
// Fixed-point sums of cloud-1 normals per cloud-2 target: integer atomics, so the same bits whatever the arrival order.
__global__ __launch_bounds__(256) void assign_kernel(const int32_t *__restrict__ nn12, const double *__restrict__ normals1,
                                                     const int32_t *__restrict__ n1s, const int32_t *__restrict__ n2s, int P,
                                                     double scale, unsigned long long *__restrict__ acc, int32_t *__restrict__ cnt) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const size_t fb = (size_t)b * P;
    if (i >= n1s[2 * b]) return;
    const int j = nn12[fb + i];
    if (j < 0 || j >= n2s[2 * b]) return;   // reported by reduce_kernel
    const double *nv = normals1 + (fb + i) * 3;
    for (int k = 0; k < 3; ++k) atomicAdd(acc + (fb + j) * 3 + k, (unsigned long long)llrint(nv[k] * scale));
    atomicAdd(cnt + fb + j, 1);
}

__device__ __forceinline__ float sqrt_rn(float d) { return (float)sqrt((double)d); }   // correctly rounded fp32 sqrt

__device__ __forceinline__ double plane_term(float px, float py, float pz, float qx, float qy, float qz, const double *n) {
    const float ex = px - qx, ey = py - qy, ez = pz - qz;   // fp32 difference, as numpy subtracts two float32 clouds
    const double dot = (((double)ex * n[0]) + ((double)ey * n[1])) + ((double)ez * n[2]);
    return dot * dot;
}

// Partial sums over EV_CHUNK points of each direction per workgroup -> part[b][chunk][8] (sums 2..9 of the header).
__global__ __launch_bounds__(256) void reduce_kernel(Cloud C1, Cloud C2, int P, const int32_t *__restrict__ nn12,
                                                     const int32_t *__restrict__ nn21, const double *__restrict__ normals1,
                                                     const unsigned long long *__restrict__ acc, const int32_t *__restrict__ cnt,
                                                     double inv_scale, float thr, int nch, double *__restrict__ part) {
    const int b = blockIdx.y, ch = blockIdx.x;
    const size_t fb = (size_t)b * P;
    const int n1 = C1.n[2 * b], n2 = C2.n[2 * b];
    double s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const bool planes = normals1 != nullptr;
    if (n1 > 0 && n2 > 0) {
        const int i1 = min(n1, (ch + 1) * EV_CHUNK);
        for (int i = ch * EV_CHUNK + threadIdx.x; i < i1; i += 256) {
            const int j = nn12[fb + i];
            if (j < 0 || j >= n2) { s[0] += NAN; continue; }
            const float *p = C1.pts + (fb + C1.pix[fb + i]) * 3, *q = C2.pts + (fb + C2.pix[fb + j]) * 3;
            const float d = dist3(q[0], q[1], q[2], p[0], p[1], p[2]);
            s[0] += sqrt_rn(d), s[2] += d, s[4] += d < thr ? 1.0 : 0.0;
            if (planes) {
                double nj[3];
                const int c = cnt[fb + j];
                if (c > 0) {
                    for (int k = 0; k < 3; ++k) nj[k] = ((double)(long long)acc[(fb + j) * 3 + k] * inv_scale) / c;
                } else {
                    const int k1 = nn21[fb + j];
                    if (k1 < 0 || k1 >= n1) { s[6] += NAN; continue; }
                    for (int k = 0; k < 3; ++k) nj[k] = normals1[(fb + k1) * 3 + k];
                }
                s[6] += plane_term(p[0], p[1], p[2], q[0], q[1], q[2], nj);
            }
        }
        const int j1 = min(n2, (ch + 1) * EV_CHUNK);
        for (int j = ch * EV_CHUNK + threadIdx.x; j < j1; j += 256) {
            const int i = nn21[fb + j];
            if (i < 0 || i >= n1) { s[1] += NAN; continue; }
            const float *p = C2.pts + (fb + C2.pix[fb + j]) * 3, *q = C1.pts + (fb + C1.pix[fb + i]) * 3;
            const float d = dist3(q[0], q[1], q[2], p[0], p[1], p[2]);
            s[1] += sqrt_rn(d), s[3] += d, s[5] += d < thr ? 1.0 : 0.0;
            if (planes) s[7] += plane_term(p[0], p[1], p[2], q[0], q[1], q[2], normals1 + (fb + i) * 3);
        }
    }
    __shared__ double sh[8][256];
    for (int k = 0; k < 8; ++k) sh[k][threadIdx.x] = s[k];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {   // fixed tree: the same order on every run
        if (threadIdx.x < o)
            for (int k = 0; k < 8; ++k) sh[k][threadIdx.x] += sh[k][threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x < 8) part[((size_t)b * nch + ch) * 8 + threadIdx.x] = sh[threadIdx.x][0];
}

__global__ void finalize_kernel(const int32_t *__restrict__ n1s, const int32_t *__restrict__ n2s, const double *__restrict__ part,
                                int nch, bool planes, double *__restrict__ sums) {
    const int b = blockIdx.x, k = threadIdx.x;
    if (k >= RPCC_EVAL_NSUMS) return;
    const int n1 = n1s[2 * b], n2 = n2s[2 * b];
    double v;
    if (k == 0) v = n1;
    else if (k == 1) v = n2;
    else if (n1 == 0 || n2 == 0 || (k >= 8 && !planes)) v = NAN;
    else {
        v = 0.0;
        for (int c = 0; c < nch; ++c) v += part[((size_t)b * nch + c) * 8 + (k - 2)];
    }
    sums[(size_t)b * RPCC_EVAL_NSUMS + k] = v;
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
struct Layout {
    int H, W, ntc, T, nch;
    size_t P, off_rank[2], off_pix[2], off_rowcnt[2], off_rowoff[2], off_n, off_tiles[2], off_acc, off_cnt, off_part, total;
};

static Layout layout(int B, int H, int W) {
    Layout L;
    L.H = H, L.W = W, L.P = (size_t)H * W;
    L.ntc = tile_cols(W);
    L.T = tile_count(H, W);
    L.nch = (int)((L.P + EV_CHUNK - 1) / EV_CHUNK);
    size_t o = 0;
    for (int c = 0; c < 2; ++c) {
        L.off_rank[c] = o, o += al((size_t)B * L.P * 4);
        L.off_pix[c] = o, o += al((size_t)B * L.P * 4);
        L.off_rowcnt[c] = o, o += al((size_t)B * H * 4);
        L.off_rowoff[c] = o, o += al((size_t)B * H * 4);
        L.off_tiles[c] = o, o += al((size_t)B * L.T * 2 * sizeof(float4));
    }
    L.off_n = o, o += al((size_t)B * 2 * 4);
    L.off_acc = o, o += al((size_t)B * L.P * 3 * 8);
    L.off_cnt = o, o += al((size_t)B * L.P * 4);
    L.off_part = o, o += al((size_t)B * L.nch * 8 * 8);
    L.total = o;
    return L;
}

static Cloud cloud(const Layout &L, char *ws, int c, const float *pts) {
    Cloud C;
    C.pts = pts;
    C.rank = (int32_t *)(ws + L.off_rank[c]);
    C.pix = (int32_t *)(ws + L.off_pix[c]);
    C.rowcnt = (int32_t *)(ws + L.off_rowcnt[c]);
    C.rowoff = (int32_t *)(ws + L.off_rowoff[c]);
    C.n = (int32_t *)(ws + L.off_n) + c;
    C.tiles = (float4 *)(ws + L.off_tiles[c]);
    return C;
}

static int prepare(const Layout &L, const Cloud &C, int B, hipStream_t st) {
    tile_box_kernel<<<dim3(L.T, B), 256, 0, st>>>(LoadPoint{C.pts}, L.H, L.W, L.ntc, L.T, C.tiles);
    row_count_kernel<<<dim3(L.H, B), 256, 0, st>>>(IsPoint{C.pts}, L.H, L.W, C.rowcnt);
    scan_kernel<2><<<B, 256, 0, st>>>(C.rowcnt, L.H, C.rowoff, C.n);
    rank_kernel<<<dim3(L.H, B), 256, 0, st>>>(C.pts, L.H, L.W, C.rowoff, C.rank, C.pix);
    LAUNCH_CHECK();
    return 0;
}

extern "C" size_t rpcc_eval_workspace_bytes(int B, int H, int W) { return shape_ok(B, H, W) ? layout(B, H, W).total : 0; }

extern "C" int rpcc_eval_nn(const float *pts1, const float *pts2, int B, int H, int W, int flags, float *dist1, int32_t *idx1,
                            float *dist2, int32_t *idx2, int32_t *n, int32_t *visits, void *ws, void *stream) {
    ARG_TRY(shape_ok(B, H, W));
    ARG_TRY(pts1 && pts2 && dist1 && idx1 && dist2 && idx2 && n && ws);
    ARG_TRY((flags & ~RPCC_EVAL_BRUTEFORCE) == 0);
    const Layout L = layout(B, H, W);
    hipStream_t st = (hipStream_t)stream;
    const Cloud C1 = cloud(L, (char *)ws, 0, pts1), C2 = cloud(L, (char *)ws, 1, pts2);
    int rc;
    if ((rc = prepare(L, C1, B, st)) || (rc = prepare(L, C2, B, st))) return rc;
    const int brute = flags & RPCC_EVAL_BRUTEFORCE;
    search_kernel<NnState, NnOut><<<dim3(L.T, B), 256, 0, st>>>(C1, C2, H, W, L.ntc, L.T, brute, 0.f, NnOut{dist1, idx1}, visits);
    search_kernel<NnState, NnOut><<<dim3(L.T, B), 256, 0, st>>>(C2, C1, H, W, L.ntc, L.T, brute, 0.f, NnOut{dist2, idx2},
                                                                 visits ? visits + L.P : nullptr);
    LAUNCH_CHECK();
    HIP_TRY(hipMemcpyAsync(n, (char *)ws + L.off_n, (size_t)B * 2 * 4, hipMemcpyDeviceToDevice, st));
    return 0;
}

extern "C" int rpcc_eval_normals(const float *pts, int B, int H, int W, double r, int flags, double *normals, int32_t *nbr, void *ws,
                                 void *stream) {
    ARG_TRY(shape_ok(B, H, W));
    ARG_TRY(pts && normals && ws);
    ARG_TRY(r > 0.0 && r * r <= 3.0e38);
    ARG_TRY((flags & ~RPCC_EVAL_BRUTEFORCE) == 0);
    const Layout L = layout(B, H, W);
    hipStream_t st = (hipStream_t)stream;
    const Cloud C = cloud(L, (char *)ws, 0, pts);
    int rc;
    if ((rc = prepare(L, C, B, st))) return rc;
    search_kernel<KnnState, KnnOut><<<dim3(L.T, B), 256, 0, st>>>(C, C, H, W, L.ntc, L.T, flags & RPCC_EVAL_BRUTEFORCE, (float)(r * r),
                                                                   KnnOut{normals, nbr}, nullptr);
    LAUNCH_CHECK();
    return 0;
}

extern "C" int rpcc_eval_metrics(const float *pts1, const float *pts2, int B, int H, int W, const int32_t *nn12, const int32_t *nn21,
                                 const double *normals1, float threshold_sq, double *sums, void *ws, void *stream) {
    ARG_TRY(shape_ok(B, H, W));
    ARG_TRY(pts1 && pts2 && nn12 && nn21 && sums && ws);
    ARG_TRY(threshold_sq >= 0.f);
    const Layout L = layout(B, H, W);
    hipStream_t st = (hipStream_t)stream;
    char *w = (char *)ws;
    const Cloud C1 = cloud(L, w, 0, pts1), C2 = cloud(L, w, 1, pts2);
    int rc;
    if ((rc = prepare(L, C1, B, st)) || (rc = prepare(L, C2, B, st))) return rc;
    // Fixed point with 61 - ceil(log2(P + 1)) fraction bits: |normal| <= 1 and at most P terms per target, so a sum stays
    // below 2^61 in magnitude; the quantum (<= 2^-34) is far below the metrics' fp64 tolerance.
    int bits = 0;
    while (((size_t)1 << bits) < L.P + 1) ++bits;
    const double scale = ldexp(1.0, 61 - bits);
    unsigned long long *acc = (unsigned long long *)(w + L.off_acc);
    int32_t *cnt = (int32_t *)(w + L.off_cnt);
    double *part = (double *)(w + L.off_part);
    if (normals1) {
        HIP_TRY(hipMemsetAsync(acc, 0, (size_t)B * L.P * 3 * 8, st));
        HIP_TRY(hipMemsetAsync(cnt, 0, (size_t)B * L.P * 4, st));
        assign_kernel<<<dim3((unsigned)((L.P + 255) / 256), B), 256, 0, st>>>(nn12, normals1, C1.n, C2.n, (int)L.P, scale, acc, cnt);
    }
    reduce_kernel<<<dim3(L.nch, B), 256, 0, st>>>(C1, C2, (int)L.P, nn12, nn21, normals1, acc, cnt, 1.0 / scale, threshold_sq, L.nch,
                                                   part);
    finalize_kernel<<<B, 64, 0, st>>>(C1.n, C2.n, part, L.nch, normals1 != nullptr, sums);
    LAUNCH_CHECK();
    return 0;
}
