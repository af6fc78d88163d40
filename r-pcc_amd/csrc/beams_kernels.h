// beams_kernels.h -- projection through a per-beam elevation table (rpcc_project_beams).
// Included by rpcc_hip.hip behind the even projection, whose helpers it shares (find_frame, fast_atan_pos, atan2f_fdlibm).
//
// replaces the table branch of PCTransformer.point_cloud_to_range_image (dataset/transformer.py:68-91), batched:
//   depth = sqrtf(x*x + y*y + z*z)                            a point whose depth is not finite is skipped
//   az    = atan2f(y, x);  az < 0: az + (float)(2 pi) in fp32  (numpy's float32 `%`; NOT the even path's double literal)
//   col   = rintf(az / hfov * W) mod W                        half to even
//   el    = atan2f(z, sqrtf(x*x + y*y))
//   row   = first arg-min over h of |va[h] - (double)el|      fp64, the table in row order
//   ri[row, col] = depth of the LAST such point in input order (a depth-0 point that comes last leaves 0)
//
// Two differences from the even path make this its own kernels: the row is a search in a table, and the write rule is
// "largest input position", not "smallest depth".  Pass 1 computes every point's pixel (screened fast path, exact sequence for
// the rest through an LDS queue drained by full workgroups, as project_pix_kernel does), remembers it (4 bytes per point) and
// takes the maximum in-frame position per pixel on an i32 [B,P] plane; pass 2 lets the point that holds the maximum write.
#pragma once

#define BEAMS_THREADS 256
#define BEAMS_PPT 4   // points per thread and chunk
#define BEAMS_SKIP 0xFFFFFFFFu   // remembered pixel of a skipped point

// Budget of the fast path.  Column: the even path's angle term plus the fp32 addition of (float)(2 pi) that the
// exact sequence rounds and the fast one does not (half an ulp at 2 pi: 2.4e-7; 5e-7 taken).  Row: the even path's elevation term
// (2e-6 + 1e-7 for the hardware square root of rho) plus the rounding of a midpoint to fp32 (half an ulp below pi/2: 6e-8) and of the
// fp64 differences the arg-min compares (below 1e-15; 1e-9 taken).
#define BEAMS_COL_ANGLE_ERR (PIX_ANGLE_ERR + 5.0e-7f)
#define BEAMS_ROW_ANGLE_ERR (PIX_ANGLE_ERR + 1.0e-7f + 6.0e-8f + 1.0e-9f)
struct BeamsFastCfg {
    float kcol, ccol, mrow;   // W / hfov; 0.5 - column margin [pixels]; elevation margin [rad]
    int on;
};
static BeamsFastCfg beams_fast_cfg(const rpcc_geom g) {
    BeamsFastCfg c;
    c.kcol = (float)g.W / g.horizontal_fov;
    const float mcol = PIX_MARGIN * (BEAMS_COL_ANGLE_ERR * fabsf(c.kcol) + PIX_REL_ERR * (float)g.W);
    c.ccol = 0.5f - mcol;
    c.mrow = PIX_MARGIN * BEAMS_ROW_ANGLE_ERR;
    c.on = (g.W >= 2 && g.horizontal_fov > 0.0f && mcol < 0.2f && mcol == mcol) ? 1 : 0;
    return c;
}

// The index in LDS (layout: beam_index.h).  row[k] >= 0: the row of sorted position k, and the fast path may answer with it; row[k] < 0: ~row[k] is
// the row, and every point located there takes the exact sequence.  That is the case where an entry lies within BEAMS_MIN_GAP of a neighbour
// (equal entries included) or beyond BEAMS_MAX_ANGLE: for an elevation on the far side of BOTH entries their fp64 distances differ by the gap
// alone, however far the elevation is from their midpoint, and a gap near the rounding of those distances (2^-53 |d|) turns into a tie that the
// first-minimum rule decides by ROW order; and a midpoint above pi/2 rounds to fp32 with more than the budget's 6e-8.
#define BEAMS_MIN_GAP 1.0e-9
#define BEAMS_MAX_ANGLE 1.6
struct BeamsTable { double va[RPCC_BEAM_MAX_H]; float mid[RPCC_BEAM_MAX_H]; int32_t row[RPCC_BEAM_MAX_H]; };
__device__ __forceinline__ void beams_table_load(BeamsTable &t, const char *__restrict__ beams, int H) {
    const double *va = reinterpret_cast<const double *>(beams);
    const float *mid = reinterpret_cast<const float *>(beams + (size_t)H * 16);
    const int32_t *row = reinterpret_cast<const int32_t *>(beams + (size_t)H * 20);
    const double *sorted = reinterpret_cast<const double *>(beams + (size_t)H * 8);
    for (int h = threadIdx.x; h < H; h += blockDim.x) {
        bool sure = fabs(sorted[h]) <= BEAMS_MAX_ANGLE;
        if (h > 0) sure = sure && sorted[h] - sorted[h - 1] > BEAMS_MIN_GAP && fabs(sorted[h - 1]) <= BEAMS_MAX_ANGLE;
        if (h < H - 1) sure = sure && sorted[h + 1] - sorted[h] > BEAMS_MIN_GAP && fabs(sorted[h + 1]) <= BEAMS_MAX_ANGLE;
        const int r = min(max(row[h], 0), H - 1);   // (a row outside the image -- an index of another H -- cannot leave it)
        t.va[h] = va[h]; t.mid[h] = mid[h]; t.row[h] = sure ? r : ~r;
    }
}

// the exact sequence; false: the point is skipped (depth not finite)
__device__ __forceinline__ bool beams_point_exact(float x, float y, float z, const rpcc_geom g, const BeamsTable &t, int &pix, float &depth) {
    depth = sqrtf(x * x + y * y + z * z);
    if (!(fabsf(depth) <= 3.402823466e+38f)) return false;
    float az = atan2f_fdlibm(y, x);
    if (az < 0) az = az + 6.28318530717958647692f;   // (float)(2 pi), fp32 addition
    const float colf = az / g.horizontal_fov * (float)g.W;
    const float cr = rintf(colf);   // half to even (the rounding mode is never changed)
    // (az >= 0 and hfov > 0: cr >= 0; a column beyond the int range -- a degenerate hfov -- saturates instead of overflowing)
    int col = cr < 2147483520.0f ? (int)cr : 2147483520;
    if (col >= g.W) col = col % g.W;
    if (col < 0) col = 0;   // (unreachable: az >= 0)
    const double el = (double)atan2f_fdlibm(z, sqrtf(x * x + y * y));
    int best = 0;
    double bd = fabs(t.va[0] - el);
    for (int h = 1; h < g.H; h++) {   // first minimum: strict <
        const double d = fabs(t.va[h] - el);
        if (d < bd) { bd = d; best = h; }
    }
    pix = best * g.W + col;
    return true;
}

// -> true when pix is certainly the exact sequence's pixel (then the depth is finite and not 0)
__device__ __forceinline__ bool beams_point_fast(float x, float y, float z, const rpcc_geom g, const BeamsFastCfg c, const BeamsTable &t, int &pix) {
    const float ax = fabsf(x), ay = fabsf(y), az = fabsf(z);
    const float mx = u2f(max(f2u(ax), f2u(ay))), mn = u2f(min(f2u(ax), f2u(ay)));
    bool ok = mx >= 1.5e-14f && ax <= 1.15e18f && ay <= 1.15e18f && az <= 1.15e18f;   // (false for NaN / inf / the origin, as in project_point_fast)
    float a = fast_atan_pos(mn, mx);
    a = ay > ax ? 1.57079633f - a : a;
    a = x < 0.0f ? 3.14159265f - a : a;
    a = y < 0.0f ? 6.28318531f - a : a;
    const float colf = a * c.kcol;
    const float c0 = rintf(colf);
    ok = ok && fabsf(colf - c0) < c.ccol && c0 >= 1.0f && c0 <= (float)(g.W - 1);   // halves, columns 0 / W: the exact way
    const float rho = __builtin_amdgcn_sqrtf(__builtin_fmaf(x, x, y * y));
    float e = fast_atan_pos(u2f(min(f2u(az), f2u(rho))), u2f(max(f2u(az), f2u(rho))));
    e = az > rho ? 1.57079633f - e : e;
    e = z < 0.0f ? -e : e;
    // k = midpoints below e = the sorted position whose interval holds e (mid[] ascends; 7 steps cover H - 1 <= 127 midpoints)
    int k = 0;
#pragma unroll
    for (int step = 64; step > 0; step >>= 1) {
        const int n = k + step;
        if (n <= g.H - 1 && t.mid[n - 1] < e) k = n;
    }
    const float below = k > 0 ? e - t.mid[k - 1] : 3.0e38f;
    const float above = t.mid[k] - e;   // (mid[H - 1] = +inf)
    const int rk = t.row[k];
    ok = ok && below > c.mrow && above > c.mrow && rk >= 0;
    pix = (rk >= 0 ? rk : ~rk) * g.W + (int)c0;
    return ok;
}

// frame of point i, for all lanes of a wavefront at once: one search for the wavefront's first point, another only in the lanes beyond that frame's end
__device__ __forceinline__ int beams_frame(const int64_t *__restrict__ offs, int B, int64_t i, int64_t wave_first) {
    int b = __builtin_amdgcn_readfirstlane(find_frame(offs, B, wave_first));
    if (i < offs[b] || i >= offs[b + 1]) b = find_frame(offs, B, i);
    return b;
}

__global__ __launch_bounds__(256) void beams_fill_kernel(int32_t *__restrict__ plane, float *__restrict__ ri, int64_t n) {
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) { plane[p] = -1; ri[p] = 0.0f; }
}

// pass 1: pixel of every point -> pixrec[i]; plane[b][pix] = max in-frame position.  total > 0.
template <int PS>
__global__ __launch_bounds__(BEAMS_THREADS) void beams_pix_kernel(const float *__restrict__ xyz, const int64_t *__restrict__ offs, int64_t total, int B,
                                                                  rpcc_geom g, BeamsFastCfg cfg, const char *__restrict__ beams,
                                                                  int32_t *__restrict__ plane, uint32_t *__restrict__ pixrec) {
    __shared__ BeamsTable t;
    __shared__ uint32_t queue[(BEAMS_PPT + 1) * BEAMS_THREADS];   // point indices (total < 2^31)
    __shared__ uint32_t qn;
    beams_table_load(t, beams, g.H);
    if (threadIdx.x == 0) qn = 0u;
    __syncthreads();
    const int64_t P = (int64_t)g.H * g.W;
    const int lane = threadIdx.x & 63;
    const unsigned long long lt = (1ull << lane) - 1ull;
    auto exact = [&](int64_t i) {
        const float x = xyz[PS * i], y = xyz[PS * i + 1], z = xyz[PS * i + 2];
        int pix;
        float depth;
        if (!beams_point_exact(x, y, z, g, t, pix, depth)) { pixrec[i] = BEAMS_SKIP; return; }
        const int b = find_frame(offs, B, i);
        pixrec[i] = (uint32_t)pix;
        atomicMax(&plane[b * P + pix], (int32_t)(i - offs[b]));
    };
    const int64_t CH = (int64_t)BEAMS_PPT * BEAMS_THREADS, nck = (total + CH - 1) / CH;
    for (int64_t k = blockIdx.x; k < nck; k += gridDim.x) {
#pragma unroll
        for (int u = 0; u < BEAMS_PPT; u++) {
            const int64_t iw = k * CH + u * BEAMS_THREADS + (threadIdx.x & ~63);   // the wavefront's first point
            const int64_t i = iw + lane;
            const bool in = i < total;
            const int64_t ic = in ? i : total - 1;   // (clamped: every lane loads a point of the launch)
            float x, y, z;
            if (PS == 4) { const float4 p4 = reinterpret_cast<const float4 *>(xyz)[ic]; x = p4.x; y = p4.y; z = p4.z; }
            else { x = xyz[3 * ic]; y = xyz[3 * ic + 1]; z = xyz[3 * ic + 2]; }
            int pix;
            const bool fast = beams_point_fast(x, y, z, g, cfg, t, pix) && cfg.on && in;
            if (iw < total) {   // (wave-uniform)
                const int b = beams_frame(offs, B, ic, iw);
                if (fast) {
                    pixrec[i] = (uint32_t)pix;
                    atomicMax(&plane[b * P + pix], (int32_t)(i - offs[b]));
                }
            }
            const bool slow = in && !fast;
            const unsigned long long sm = __ballot(slow);
            if (sm) {
                const int leader = (int)__ffsll((long long)sm) - 1;
                uint32_t q0 = 0u;
                if (lane == leader) q0 = atomicAdd(&qn, (uint32_t)__popcll(sm));
                q0 = (uint32_t)__builtin_amdgcn_readlane((int)q0, leader);
                if (slow) queue[q0 + __popcll(sm & lt)] = (uint32_t)i;
            }
        }
        __syncthreads();
        uint32_t n = qn;
        __syncthreads();
        if (n >= BEAMS_THREADS) {   // full workgroups of uncertain points: the exact sequence
            while (n >= BEAMS_THREADS) {
                exact((int64_t)queue[n - BEAMS_THREADS + threadIdx.x]);
                n -= BEAMS_THREADS;
            }
            __syncthreads();
            if (threadIdx.x == 0) qn = n;
            __syncthreads();
        }
    }
    const uint32_t n = qn;
    if (threadIdx.x < n) exact((int64_t)queue[threadIdx.x]);
}

// pass 2: the point that holds its pixel's maximum writes its depth (one writer per pixel)
__global__ __launch_bounds__(256) void beams_write_kernel(const float *__restrict__ xyz, const int64_t *__restrict__ offs, int64_t total, int B, int64_t P,
                                                          const int32_t *__restrict__ plane, const uint32_t *__restrict__ pixrec,
                                                          float *__restrict__ ri, int ps) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63); i0 < total; i0 += stride) {   // (i0: wave-uniform)
        const int64_t i = i0 + (threadIdx.x & 63);
        if (i >= total) continue;
        const uint32_t pr = pixrec[i];
        const int b = beams_frame(offs, B, i, i0);
        if (pr == BEAMS_SKIP) continue;
        if (plane[b * P + pr] != (int32_t)(i - offs[b])) continue;
        const float x = xyz[ps * i], y = xyz[ps * i + 1], z = xyz[ps * i + 2];
        ri[b * P + pr] = sqrtf(x * x + y * y + z * z);
    }
}

// test hook: counts[0] = points the fast path is certain about, counts[1] = of those, points the exact sequence skips or puts elsewhere
// (must be 0), counts[2] = points sent to the exact sequence
__global__ __launch_bounds__(256) void beams_check_kernel(const float *__restrict__ xyz, int64_t total, rpcc_geom g, BeamsFastCfg cfg,
                                                          const char *__restrict__ beams, unsigned long long *__restrict__ counts) {
    __shared__ BeamsTable t;
    beams_table_load(t, beams, g.H);
    __syncthreads();
    int sure = 0, bad = 0, slow = 0;   // (per thread: at most total / (grid x 256) + 1 points)
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
        int pf, pe = -1;
        float depth = 0.0f;
        const bool ok = beams_point_fast(x, y, z, g, cfg, t, pf) && cfg.on;
        const bool kept = beams_point_exact(x, y, z, g, t, pe, depth);
        if (ok) { sure++; if (!kept || depth == 0.0f || pe != pf) bad++; } else slow++;
    }
    const int s = wave_sum_i32(sure), b2 = wave_sum_i32(bad), sl = wave_sum_i32(slow);
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&counts[0], (unsigned long long)s);
        atomicAdd(&counts[1], (unsigned long long)b2);
        atomicAdd(&counts[2], (unsigned long long)sl);
    }
}

// Scratch: plane i32 [B,P] | remembered pixels u32 [total].  Neither needs initialisation: the fill kernel writes every word of the
// plane, pass 1 every remembered pixel that pass 2 reads.
struct BeamsLayout { int32_t *plane; uint32_t *pixrec; size_t bytes; };
static BeamsLayout beams_layout(void *scratch, int64_t total, int B, int P) {
    Carve c(scratch);
    BeamsLayout l;
    l.plane = c.take<int32_t>((size_t)B * P * 4);
    l.pixrec = c.take<uint32_t>((size_t)(total > 0 ? total : 0) * 4);
    l.bytes = round_up(c.bytes(), 256);
    return l;
}

static int beams_args_ok(int64_t total, int B, rpcc_geom g) {
    ARG_TRY(B > 0 && B <= RPCC_MAX_BATCH && g.H >= 1 && g.H <= RPCC_BEAM_MAX_H && g.W > 0 && total >= 0 && total < ((int64_t)1 << 31));
    ARG_TRY(g.horizontal_fov > 0.0f && (int64_t)g.H * g.W < ((int64_t)1 << 31) && (int64_t)B * g.H * g.W < ((int64_t)1 << 40));   // (P is an int)
    return RPCC_OK;
}

// On return (of the stream) ri is final: the last point's depth per pixel, 0 where no point fell.
static int launch_project_beams(const float *xyz, const int64_t *offsets, int64_t total, int B, rpcc_geom g, const void *beams, float *ri,
                                void *scratch, size_t scratch_bytes, hipStream_t st, int ps) {
    const int P = g.H * g.W;
    const BeamsLayout l = beams_layout(scratch, total, B, P);
    ARG_TRY(scratch_bytes >= l.bytes);
    const int64_t n = (int64_t)B * P;
    beams_fill_kernel<<<(unsigned)std::min<int64_t>((n + 255) / 256, 8192), 256, 0, st>>>(l.plane, ri, n);
    LAUNCH_CHECK();
    if (total == 0) return RPCC_OK;
    const int64_t nck = (total + BEAMS_PPT * BEAMS_THREADS - 1) / (BEAMS_PPT * BEAMS_THREADS);
    const unsigned wgs = (unsigned)std::min<int64_t>(nck, 256 * 8);
    const char *bt = reinterpret_cast<const char *>(beams);
    if (ps == 4) beams_pix_kernel<4><<<wgs, BEAMS_THREADS, 0, st>>>(xyz, offsets, total, B, g, beams_fast_cfg(g), bt, l.plane, l.pixrec);
    else beams_pix_kernel<3><<<wgs, BEAMS_THREADS, 0, st>>>(xyz, offsets, total, B, g, beams_fast_cfg(g), bt, l.plane, l.pixrec);
    LAUNCH_CHECK();
    beams_write_kernel<<<(unsigned)std::min<int64_t>((total + 255) / 256, 8192), 256, 0, st>>>(xyz, offsets, total, B, (int64_t)P, l.plane, l.pixrec, ri, ps);
    LAUNCH_CHECK();
    return RPCC_OK;
}

extern "C" size_t rpcc_beam_index_bytes(int H) { return H >= 1 && H <= RPCC_BEAM_MAX_H ? RPCC_BEAM_INDEX_BYTES(H) : 0; }
extern "C" int rpcc_beam_index_build(const double *angles, int H, void *out) {
    if (rpcc_beam_index_build_impl(angles, H, out) != 0)
        return set_err(RPCC_ERR_ARG, "rpcc_beam_index_build: 1 <= H <= 128 finite angles and an output buffer are needed%s%s");
    return RPCC_OK;
}
extern "C" size_t rpcc_project_beams_scratch_bytes(int64_t total, int B, int P) {
    return B > 0 && P > 0 && total >= 0 ? beams_layout(nullptr, total, B, P).bytes : 0;
}
extern "C" int rpcc_project_beams(const float *points, int point_stride_bytes, const int64_t *offsets, int64_t total, int B, rpcc_geom g,
                                  const void *beams_dev, float *ri, void *scratch, size_t scratch_bytes, void *stream) {
    int rc;
    if ((rc = beams_args_ok(total, B, g))) return rc;
    ARG_TRY(ri != nullptr && scratch != nullptr && offsets != nullptr && beams_dev != nullptr);
    ARG_TRY(total == 0 || points != nullptr);
    ARG_TRY(point_floats(point_stride_bytes) > 0);
    ARG_TRY(point_stride_bytes != 16 || (reinterpret_cast<uintptr_t>(points) & 15u) == 0);   // rows are read with 16-byte loads
    ARG_TRY((reinterpret_cast<uintptr_t>(beams_dev) & 7u) == 0);
    return launch_project_beams(points, offsets, total, B, g, beams_dev, ri, scratch, scratch_bytes, (hipStream_t)stream, point_floats(point_stride_bytes));
}
extern "C" int rpcc_project_beams_check(const float *xyz, int64_t total, rpcc_geom g, const void *beams_dev, uint64_t *counts, void *stream) {
    int rc;
    if ((rc = beams_args_ok(total, 1, g))) return rc;
    ARG_TRY(xyz && counts && beams_dev && total > 0 && (reinterpret_cast<uintptr_t>(beams_dev) & 7u) == 0);
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(counts, 0, 3 * sizeof(uint64_t), st));
    beams_check_kernel<<<2048, 256, 0, st>>>(xyz, total, g, beams_fast_cfg(g), reinterpret_cast<const char *>(beams_dev),
                                             reinterpret_cast<unsigned long long *>(counts));
    LAUNCH_CHECK();
    return RPCC_OK;
}
