// The points that share a pixel through the codec (include/rpcc_hip.h "hidden_points"; the specification is stated once, in
// tests/hidden_ref.py).  Included from rpcc_hip.hip behind the subpixel section: the owner of a pixel is the intensity channel's
// (intensity_owner_pass), every point goes through project_point, the exact sequence that produced ri, and the lateral codes are
// subpixel_code of the point's own offsets.
//
//   owner pass      intensity_kernels.h, over this entry's own scratch.
//   count pass      grid-stride over the rows: a row of finite, non-zero depth that is not its pixel's owner is a hidden point; one in an
//                   empty pixel or with a range code past 65535 adds to its frame's uncarried counter, every other one stores its key
//                   (k << 8 | az << 4 | el) and its pixel and adds to the pixel's counter.
//   scan pass       one workgroup per frame, raster order: the counters into segment starts, min(count, 255) into final starts, the rank
//                   among the non-empty pixels; header, count plane, nbytes, orphans, uncarried.
//   scatter pass    every hidden point takes a slot of its pixel's segment with an atomic cursor.
//   rank pass       one thread per slot: its rank inside the segment by (key, slot); ranks below 255 go to the final start + rank.  Equal
//                   keys are interchangeable, so the bytes do not depend on which thread took which slot.
//   decode pass     one workgroup per frame: every check before anything is written, then the count plane is scanned into starts and
//                   every pixel writes its points: r * tm (bits 0) or the pixel's ray turned by the offsets (subpixel_turn_ray).
#define HID_MAGIC 0x31485052u   // "RPH1", little-endian
#define HID_THREADS 256
#define HID_HEADER 16
#define HID_CAP 255             // carried hidden points per pixel: the count plane holds one byte
#define HID_NONE (-1)
#define HID_INFO 4              // uint32 per frame: n, m, hidden points counted, 1 when the payload fits its row

struct HiddenLayout {
    IntensityLayout own;
    uint32_t *zeroed, *cnt, *cursor, *lost;   // zeroed: cnt [B P], cursor [B P], lost [B] in one run
    size_t zeroed_bytes;
    uint32_t *start, *fstart, *info, *keys, *skey;
    int32_t *pix, *spix;
    size_t bytes;
};
static HiddenLayout hidden_layout(void *scratch, int B, int P, int64_t total) {
    HiddenLayout l;
    l.own = intensity_layout(scratch, B, P);
    Carve c(scratch);
    (void)c.take<char>(l.own.bytes, 4);                // the owner pass's regions, as rpcc_intensity_encode lays them out
    const size_t px = (size_t)B * P, rows = (size_t)(total > 0 ? total : 0);
    l.zeroed_bytes = (2 * px + (size_t)B) * 4;
    l.zeroed = c.take<uint32_t>(l.zeroed_bytes, 4);
    l.cnt = l.zeroed;                                  // hidden points per pixel (carried or past the cap)
    l.cursor = l.zeroed + px;                          // slots handed out per pixel
    l.lost = l.zeroed + 2 * px;                        // per frame: hidden points in empty pixels or with k > 65535
    l.start = c.take<uint32_t>(px * 4, 4);             // exclusive scan of cnt inside the frame
    l.fstart = c.take<uint32_t>(px * 4, 4);            // exclusive scan of min(cnt, 255)
    l.info = c.take<uint32_t>((size_t)B * HID_INFO * 4, 4);
    l.keys = c.take<uint32_t>(rows * 4, 4);            // per row: its key
    l.pix = c.take<int32_t>(rows * 4, 4);              // per row: its pixel inside the frame, HID_NONE when it is not carried
    l.skey = c.take<uint32_t>(rows * 4, 4);            // per slot (frame b's slots start at offsets[b]): key and pixel
    l.spix = c.take<int32_t>(rows * 4, 4);
    l.bytes = round_up(c.bytes(), 256);
    return l;
}

__global__ __launch_bounds__(HID_THREADS) void hidden_count_kernel(const float4 *__restrict__ rows, const int64_t *__restrict__ offs, int64_t total, int B,
                                                                   rpcc_geom g, const float *__restrict__ ri, const int32_t *__restrict__ owner, float step,
                                                                   int bits, uint32_t *__restrict__ cnt, uint32_t *__restrict__ lost,
                                                                   uint32_t *__restrict__ keys, int32_t *__restrict__ pixof) {
    const int64_t P = (int64_t)g.H * g.W;
    const int64_t lo = offs[0], hi = min(offs[B], total);   // rows outside the frames belong to nobody
    const int L = 1 << bits;
    for (int64_t i = (int64_t)blockIdx.x * HID_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * HID_THREADS) {
        int32_t px = HID_NONE;
        if (i >= lo && i < hi) {
            const float4 p = rows[i];
            const RowCol rc = project_point(p.x, p.y, p.z, g);
            if (fabsf(rc.depth) <= 3.402823466e+38f && rc.depth != 0.0f) {   // NaN / inf / 0 depth: skipped, as rpcc_project skips it
                const int b = find_frame(offs, B, i);
                const int64_t at = (int64_t)b * P + rc.pix;
                if (ri[at] == 0.0f) atomicAdd(&lost[b], 1u);                 // an empty pixel carries nothing
                else if (owner[at] != (int32_t)(i - offs[b])) {
                    const float kf = rintf(rc.depth / step);                 // one IEEE division, half to even
                    if (!(kf <= 65535.0f)) atomicAdd(&lost[b], 1u);
                    else {
                        uint32_t az = 0u, el = 0u;
                        if (bits > 0) {   // subpixel_code_kernel's expressions, on this point's own row
                            az = subpixel_code(rc.colf - roundf(rc.colf), L);
                            el = subpixel_code(rc.rowf - (float)(rc.pix / g.W), L);
                        }
                        keys[i] = (uint32_t)kf << 8 | az << 4 | el;
                        px = rc.pix;
                        atomicAdd(&cnt[at], 1u);
                    }
                }
            }
        }
        pixof[i] = px;
    }
}

__global__ __launch_bounds__(INT_FRAME_THREADS) void hidden_scan_kernel(const int64_t *__restrict__ offs, int64_t total, int P, const float *__restrict__ ri,
                                                                         const int32_t *__restrict__ owner, const uint32_t *__restrict__ cnt,
                                                                         const uint32_t *__restrict__ lostctr, float step, int bits,
                                                                         uint32_t *__restrict__ start, uint32_t *__restrict__ fstart, uint32_t *__restrict__ info,
                                                                         uint8_t *__restrict__ payload, int64_t stride, int32_t *__restrict__ nbytes,
                                                                         int32_t *__restrict__ orphans, int32_t *__restrict__ uncarried) {
    __shared__ uint32_t wsum[INT_FRAME_THREADS / 64];
    __shared__ uint32_t lost, over;
    const int b = blockIdx.x;
    if (threadIdx.x == 0) { lost = 0u; over = 0u; }
    const int64_t px0 = (int64_t)b * P, first = offs[b], end = min(offs[b + 1], total);
    uint8_t *out = payload + (int64_t)b * stride;
    uint32_t run_n = 0u, run_c = 0u, run_m = 0u, mylost = 0u, myover = 0u;
    for (int r0 = 0; r0 < P; r0 += INT_FRAME_THREADS * INT_PPT) {   // (workgroup-uniform)
        const int p0 = r0 + (int)threadIdx.x * INT_PPT;
        bool set[INT_PPT];
        uint32_t c[INT_PPT], ns = 0u, cs = 0u, ms = 0u;
#pragma unroll
        for (int k = 0; k < INT_PPT; k++) {
            set[k] = p0 + k < P && ri[px0 + p0 + k] != 0.0f;
            c[k] = set[k] ? cnt[px0 + p0 + k] : 0u;
            ns += set[k] ? 1u : 0u;
            cs += c[k];
            ms += min(c[k], (uint32_t)HID_CAP);
        }
        uint32_t all_n, all_c, all_m;
        uint32_t rank = run_n + intensity_block_scan(ns, wsum, all_n);
        uint32_t s = run_c + intensity_block_scan(cs, wsum, all_c);
        uint32_t f = run_m + intensity_block_scan(ms, wsum, all_m);
#pragma unroll
        for (int k = 0; k < INT_PPT; k++) {
            if (p0 + k >= P) continue;
            start[px0 + p0 + k] = s;
            fstart[px0 + p0 + k] = f;
            if (!set[k]) continue;
            const int32_t own = owner[px0 + p0 + k];
            const int64_t row = first + own;
            if (own == INT_NO_OWNER || row < 0 || row < first || row >= end) mylost++;   // ri is not the image of these rows
            const uint32_t carried = min(c[k], (uint32_t)HID_CAP);
            out[HID_HEADER + rank] = (uint8_t)carried;   // rank < n <= P: inside the row of at least 16 + P bytes
            myover += c[k] - carried;
            s += c[k];
            f += carried;
            rank++;
        }
        run_n += all_n; run_c += all_c; run_m += all_m;
    }
    if (mylost) atomicAdd(&lost, mylost);
    if (myover) atomicAdd(&over, myover);
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t sb = f2u(step), m = run_m;
        const int64_t len = (int64_t)HID_HEADER + run_n + (int64_t)(bits > 0 ? 4 : 2) * m;
        const bool fits = len <= stride;
        out[0] = 'R'; out[1] = 'P'; out[2] = 'H'; out[3] = '1';
        out[4] = (uint8_t)bits; out[5] = 0; out[6] = 0; out[7] = 0;
        out[8] = (uint8_t)sb; out[9] = (uint8_t)(sb >> 8); out[10] = (uint8_t)(sb >> 16); out[11] = (uint8_t)(sb >> 24);
        out[12] = (uint8_t)m; out[13] = (uint8_t)(m >> 8); out[14] = (uint8_t)(m >> 16); out[15] = (uint8_t)(m >> 24);
        info[b * HID_INFO] = run_n; info[b * HID_INFO + 1] = m; info[b * HID_INFO + 2] = run_c; info[b * HID_INFO + 3] = fits ? 1u : 0u;
        nbytes[b] = fits ? (int32_t)len : -1;   // -1: the caller's row is too short for this frame; no code of it is written
        orphans[b] = (int32_t)lost;
        uncarried[b] = (int32_t)(lostctr[b] + over);
    }
}

__global__ __launch_bounds__(HID_THREADS) void hidden_scatter_kernel(const int64_t *__restrict__ offs, int64_t total, int B, int64_t P,
                                                                     const uint32_t *__restrict__ keys, const int32_t *__restrict__ pixof,
                                                                     const uint32_t *__restrict__ start, uint32_t *__restrict__ cursor,
                                                                     uint32_t *__restrict__ skey, int32_t *__restrict__ spix) {
    for (int64_t i = (int64_t)blockIdx.x * HID_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * HID_THREADS) {
        const int32_t px = pixof[i];
        if (px == HID_NONE) continue;
        const int b = find_frame(offs, B, i);
        const int64_t at = (int64_t)b * P + px;
        // the frame's hidden points are rows of [offs[b], min(offs[b + 1], total)), each takes one slot: j stays inside that range
        const int64_t j = offs[b] + start[at] + atomicAdd(&cursor[at], 1u);
        skey[j] = keys[i];
        spix[j] = px;
    }
}

__global__ __launch_bounds__(HID_THREADS) void hidden_rank_kernel(const int64_t *__restrict__ offs, int64_t total, int B, int64_t P,
                                                                  const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ start,
                                                                  const uint32_t *__restrict__ fstart, const uint32_t *__restrict__ info,
                                                                  const uint32_t *__restrict__ skey, const int32_t *__restrict__ spix, int bits,
                                                                  uint8_t *__restrict__ payload, int64_t stride) {
    const int64_t lo = offs[0], hi = min(offs[B], total);
    for (int64_t j = (int64_t)blockIdx.x * HID_THREADS + threadIdx.x; j < total; j += (int64_t)gridDim.x * HID_THREADS) {
        if (j < lo || j >= hi) continue;
        const int b = find_frame(offs, B, j);
        const uint32_t *fi = info + b * HID_INFO;
        if (j - offs[b] >= (int64_t)fi[2] || fi[3] == 0u) continue;   // not a slot of this frame, or the row is too short
        const int64_t at = (int64_t)b * P + spix[j];
        const int64_t s0 = offs[b] + start[at], s1 = s0 + cnt[at];
        const uint32_t mine = skey[j];
        uint32_t rank = 0u;
        for (int64_t e = s0; e < s1 && rank < HID_CAP; e++) {   // the segment's own threads share the quadratic work; a wavefront reads one entry at a time
            const uint32_t other = skey[e];
            rank += other < mine || (other == mine && e < j) ? 1u : 0u;
        }
        if (rank >= HID_CAP) continue;
        const int64_t n = fi[0], m = fi[1], d = (int64_t)fstart[at] + rank;   // d < m; 16 + n + 4 m <= stride (fits)
        uint8_t *out = payload + (int64_t)b * stride + HID_HEADER + n;
        const uint32_t k = mine >> 8;
        out[2 * d] = (uint8_t)k;
        out[2 * d + 1] = (uint8_t)(k >> 8);
        if (bits > 0) {
            out[2 * m + d] = (uint8_t)(mine >> 4 & 15u);
            out[3 * m + d] = (uint8_t)(mine & 15u);
        }
    }
}

// tm: f32 [P,3] the transform map (bits 0); tables: subpixel_decode_kernel's (bits > 0).  points: f32 [B, cap, 3]
template <class L>
__global__ __launch_bounds__(INT_FRAME_THREADS) void hidden_decode_kernel(const uint8_t *__restrict__ payload, int64_t stride, const int32_t *__restrict__ nbytes,
                                                                           const L *__restrict__ labels, const float *__restrict__ tm,
                                                                           const double *__restrict__ tables, int H, int W, int64_t cap,
                                                                           float *__restrict__ points, int32_t *__restrict__ count, int32_t *__restrict__ status) {
    __shared__ uint32_t wsum[INT_FRAME_THREADS / 64];
    const int b = blockIdx.x;
    const int P = H * W;
    const int64_t px0 = (int64_t)b * P;
    const uint8_t *in = payload + (int64_t)b * stride;
    const int64_t nb = nbytes[b];
    // the header is read only when the row holds one
    bool ok = nb >= HID_HEADER && nb <= stride;
    int bits = 0;
    float step = 1.0f;
    int64_t m = 0;
    if (ok) {
        const uint32_t magic = (uint32_t)in[0] | (uint32_t)in[1] << 8 | (uint32_t)in[2] << 16 | (uint32_t)in[3] << 24;
        bits = in[4];
        step = u2f((uint32_t)in[8] | (uint32_t)in[9] << 8 | (uint32_t)in[10] << 16 | (uint32_t)in[11] << 24);
        m = (int64_t)((uint32_t)in[12] | (uint32_t)in[13] << 8 | (uint32_t)in[14] << 16 | (uint32_t)in[15] << 24);
        ok = magic == HID_MAGIC && bits <= 4 && in[5] == 0 && in[6] == 0 && in[7] == 0 && step > 0.0f && step <= 3.402823466e+38f && m <= cap &&
             (bits == 0 || tables != nullptr);
    }
    if (!ok) { bits = 0; m = 0; }   // (nothing is read through them then)
    // the number of pixels with a label other than 1 is what the count plane must hold
    uint32_t mine = 0u;
    for (int p = threadIdx.x; p < P; p += INT_FRAME_THREADS) mine += labels[px0 + p] != (L)1 ? 1u : 0u;
    uint32_t n;
    (void)intensity_block_scan(mine, wsum, n);
    ok = ok && nb == (int64_t)HID_HEADER + n + (int64_t)(bits > 0 ? 4 : 2) * m;   // (workgroup-uniform)
    // the counts sum to m and every lateral code is below 2^bits, or nothing of the frame is decoded (a count bounds a write, a code is an index)
    uint32_t sum = 0u;
    int bad = 0;
    if (ok) {
        for (int64_t k = threadIdx.x; k < (int64_t)n; k += INT_FRAME_THREADS) sum += in[HID_HEADER + k];   // 16 + k < nb <= stride; a thread's share: < 2^20 * 255
        if (bits > 0) {
            const uint32_t Lc = 1u << bits;
            const uint8_t *lat = in + HID_HEADER + n + 2 * m;
            for (int64_t k = threadIdx.x; k < 2 * m; k += INT_FRAME_THREADS) bad |= lat[k] >= Lc ? 1 : 0;
        }
    }
    // the workgroup's sum in 64 bits (n < 2^30 counts of up to 255 do not fit 32): the low and the high halves of the threads' shares apart
    uint32_t sum_lo, sum_hi;
    (void)intensity_block_scan(sum & 0xFFFFu, wsum, sum_lo);
    (void)intensity_block_scan(sum >> 16, wsum, sum_hi);
    ok = !__syncthreads_or(bad) && ok && (int64_t)sum_lo + ((int64_t)sum_hi << 16) == m;
    const uint8_t *rng = in + HID_HEADER + n, *azp = rng + 2 * m, *elp = azp + m;
    const double *ca = tables, *sa = tables + H, *cz = tables + 2 * H, *sz = tables + 2 * H + W;
    const double *steps = tables + 2 * H + 2 * W + (int64_t)(bits > 0 ? bits - 1 : 0) * SUB_TABLE_CODES * 4;
    float *o = points + (int64_t)b * cap * 3;
    uint32_t run_n = 0u, run_c = 0u;
    if (ok)   // (workgroup-uniform)
        for (int r0 = 0; r0 < P; r0 += INT_FRAME_THREADS * INT_PPT) {
            const int p0 = r0 + (int)threadIdx.x * INT_PPT;
            bool set[INT_PPT];
            uint32_t ns = 0u;
#pragma unroll
            for (int k = 0; k < INT_PPT; k++) {
                set[k] = p0 + k < P && labels[px0 + p0 + k] != (L)1;
                ns += set[k] ? 1u : 0u;
            }
            uint32_t all_n, all_c;
            uint32_t rank = run_n + intensity_block_scan(ns, wsum, all_n);
            uint32_t c[INT_PPT], cs = 0u;
#pragma unroll
            for (int k = 0; k < INT_PPT; k++) {
                c[k] = set[k] ? in[HID_HEADER + rank] : 0u;   // rank < n
                rank += set[k] ? 1u : 0u;
                cs += c[k];
            }
            uint32_t s = run_c + intensity_block_scan(cs, wsum, all_c);
#pragma unroll
            for (int k = 0; k < INT_PPT; k++) {
                const int p = p0 + k;
                for (uint32_t t = 0; t < c[k]; t++, s++) {   // s < m <= cap: the counts sum to m
                    const float r = (float)((uint32_t)rng[2 * (int64_t)s] | (uint32_t)rng[2 * (int64_t)s + 1] << 8) * step;
                    float x, y, z;
                    if (bits == 0) { x = r * tm[3 * p]; y = r * tm[3 * p + 1]; z = r * tm[3 * p + 2]; }
                    else subpixel_turn_ray(ca, sa, cz, sz, steps, p / W, p % W, azp[s], elp[s], (double)r, x, y, z);
                    o[3 * (int64_t)s] = x; o[3 * (int64_t)s + 1] = y; o[3 * (int64_t)s + 2] = z;
                }
            }
            run_n += all_n; run_c += all_c;
        }
    if (threadIdx.x == 0) {
        count[b] = ok ? (int32_t)m : 0;
        status[b] = ok ? RPCC_STREAM_OK : RPCC_STREAM_E_HIDDEN;
    }
}
