// Sub-pixel ray angles through the codec (include/rpcc_hip.h "subpixel"; the specification is stated once, in tests/subpixel_ref.py).
// Included from rpcc_hip.hip behind the intensity section: the owner of a pixel is the intensity channel's (intensity_owner_pass), and
// the offsets come from project_point, the exact sequence that produced ri.
//
//   owner pass      intensity_kernels.h, over this entry's own scratch.
//   code pass       grid-stride over the B * P pixels: a non-empty pixel's owner row goes through project_point once more; the two values
//                   it hands to roundf give off_az (before the wrap) and off_el (after the clamp), each quantised to `bits` bits.  One
//                   (az, el) byte pair per pixel, 0 where the pixel is empty or has no owner.
//   pack pass       one workgroup per frame, raster order: count the non-empty pixels, then rank them by the workgroup scan and store the
//                   two planes behind the header; nbytes, orphans.
//   decode pass     one workgroup per frame: header, count of labels != 1 and "every code < L" are checked before anything is written,
//                   then the same scan spreads the codes over the pixels: the ray of pixel (h, w) turned by the two reconstructed
//                   offsets through the angle-sum formulas in fp64 (no trigonometry on the device), times the range.  A refused frame
//                   is written as zeros.
#define SUB_MAGIC 0x31535052u   // "RPS1", little-endian
#define SUB_THREADS 256
#define SUB_TABLE_CODES 16      // codes per bits row of the table (L <= 16)

struct SubpixelLayout { IntensityLayout own; uint8_t *codes; size_t bytes; };
static SubpixelLayout subpixel_layout(void *scratch, int B, int P) {
    SubpixelLayout l;
    l.own = intensity_layout(scratch, B, P);
    Carve c(scratch);
    (void)c.take<char>(l.own.bytes, 4);                // the owner pass's regions, as rpcc_intensity_encode lays them out
    l.codes = c.take<uint8_t>((size_t)B * P * 2, 4);   // (az, el) per pixel where the caller gives no `codes`
    l.bytes = round_up(c.bytes(), 256);
    return l;
}

// c of tests/subpixel_ref.py: t = (off + 0.5f) * L, one fp32 add and one fp32 multiply; floor, clamped to 0 .. L - 1
__device__ __forceinline__ uint32_t subpixel_code(float off, int L) {
    const float t = (off + 0.5f) * (float)L;
    if (!(t >= 0.0f)) return 0u;
    if (t >= (float)L) return (uint32_t)(L - 1);
    return (uint32_t)(int)floorf(t);
}

__global__ __launch_bounds__(SUB_THREADS) void subpixel_code_kernel(const float4 *__restrict__ rows, const int64_t *__restrict__ offs, int64_t total,
                                                                    int B, rpcc_geom g, const float *__restrict__ ri,
                                                                    const int32_t *__restrict__ owner, int bits, uchar2 *__restrict__ codes) {
    const int64_t P = (int64_t)g.H * g.W, n = (int64_t)B * P;
    const int L = 1 << bits;
    for (int64_t i = (int64_t)blockIdx.x * SUB_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * SUB_THREADS) {
        uchar2 c = make_uchar2(0, 0);
        if (ri[i] != 0.0f) {
            const int b = (int)(i / P);
            const int32_t own = owner[i];
            const int64_t first = offs[b], end = min(offs[b + 1], total), row = first + own;
            if (own != INT_NO_OWNER && row >= 0 && row >= first && row < end) {   // (else an orphan: the pack pass counts it)
                const float4 p = rows[row];
                const RowCol rc = project_point(p.x, p.y, p.z, g);
                const float off_az = rc.colf - roundf(rc.colf);                       // before the wrap: a point that rounds to column W is negative
                const float off_el = rc.rowf - (float)(rc.pix / g.W);                 // after the clamp: may lie outside +-0.5
                c = make_uchar2((unsigned char)subpixel_code(off_az, L), (unsigned char)subpixel_code(off_el, L));
            }
        }
        codes[i] = c;
    }
}

__global__ __launch_bounds__(INT_FRAME_THREADS) void subpixel_pack_kernel(const int64_t *__restrict__ offs, int64_t total, int P, const float *__restrict__ ri,
                                                                           const int32_t *__restrict__ owner, const uchar2 *__restrict__ codes, int bits,
                                                                           uint8_t *__restrict__ payload, int64_t stride, int32_t *__restrict__ nbytes,
                                                                           int32_t *__restrict__ orphans) {
    __shared__ uint32_t wsum[INT_FRAME_THREADS / 64];
    __shared__ uint32_t lost;
    const int b = blockIdx.x;
    if (threadIdx.x == 0) lost = 0u;
    const int64_t px0 = (int64_t)b * P, first = offs[b], end = min(offs[b + 1], total);
    uint8_t *out = payload + (int64_t)b * stride;
    // the planes' length first: the el plane starts behind the az plane
    uint32_t mine = 0u;
    for (int p = threadIdx.x; p < P; p += INT_FRAME_THREADS) mine += ri[px0 + p] != 0.0f ? 1u : 0u;
    uint32_t n;
    (void)intensity_block_scan(mine, wsum, n);
    uint32_t running = 0u, mylost = 0u;
    for (int r0 = 0; r0 < P; r0 += INT_FRAME_THREADS * INT_PPT) {   // (workgroup-uniform)
        const int p0 = r0 + (int)threadIdx.x * INT_PPT;
        bool set[INT_PPT];
        uint32_t cnt = 0u;
#pragma unroll
        for (int k = 0; k < INT_PPT; k++) {
            set[k] = p0 + k < P && ri[px0 + p0 + k] != 0.0f;
            cnt += set[k] ? 1u : 0u;
        }
        uint32_t all;
        uint32_t rank = running + intensity_block_scan(cnt, wsum, all);
#pragma unroll
        for (int k = 0; k < INT_PPT; k++) {
            if (!set[k]) continue;
            const int32_t own = owner[px0 + p0 + k];
            const int64_t row = first + own;
            if (own == INT_NO_OWNER || row < 0 || row < first || row >= end) mylost++;   // ri is not the image of these rows
            const uchar2 c = codes[px0 + p0 + k];
            out[8 + rank] = c.x;          // rank < n <= P: inside the row of 8 + 2 P bytes
            out[8 + n + rank] = c.y;
            rank++;
        }
        running += all;
    }
    if (mylost) atomicAdd(&lost, mylost);
    __syncthreads();
    if (threadIdx.x == 0) {
        out[0] = 'R'; out[1] = 'P'; out[2] = 'S'; out[3] = '1';
        out[4] = (uint8_t)bits; out[5] = 0; out[6] = 0; out[7] = 0;
        nbytes[b] = 8 + 2 * (int32_t)n;
        orphans[b] = (int32_t)lost;
    }
}

// the ray of pixel (h, w) turned by the offsets the codes (a, e) stand for, times the range r: the angle sums in fp64, every product and
// sum rounded on its own (step: the table row of this bits); shared by the subpixel decoder and the hidden-points decoder
__device__ __forceinline__ void subpixel_turn_ray(const double *__restrict__ ca, const double *__restrict__ sa, const double *__restrict__ cz,
                                                  const double *__restrict__ sz, const double *__restrict__ step, int h, int w, uint32_t a, uint32_t e,
                                                  double r, float &x, float &y, float &z) {
    const double cde = step[4 * e], sde = step[4 * e + 1], cda = step[4 * a + 2], sda = step[4 * a + 3];
    const double cosalt = ca[h] * cde - sa[h] * sde, sinalt = sa[h] * cde + ca[h] * sde;
    const double cosaz = cz[w] * cda - sz[w] * sda, sinaz = sz[w] * cda + cz[w] * sda;
    x = (float)(r * (cosalt * cosaz));
    y = (float)(r * (cosalt * sinaz));
    z = (float)(r * sinalt);
}

// tables: f64 [2 H + 2 W + 4 * SUB_TABLE_CODES * 4] = ca [H], sa [H], cz [W], sz [W], then per bits 1 .. 4 and code c: cos / sin of the
// elevation step, cos / sin of the azimuth step (ops.subpixel_tables)
template <class L>
__global__ __launch_bounds__(INT_FRAME_THREADS) void subpixel_decode_kernel(const uint8_t *__restrict__ payload, int64_t stride, const int32_t *__restrict__ nbytes,
                                                                             const L *__restrict__ labels, const float *__restrict__ ri_rec,
                                                                             const double *__restrict__ tables, int H, int W, float *__restrict__ points,
                                                                             int32_t *__restrict__ status) {
    __shared__ uint32_t wsum[INT_FRAME_THREADS / 64];
    const int b = blockIdx.x;
    const int P = H * W;
    const int64_t px0 = (int64_t)b * P;
    const uint8_t *in = payload + (int64_t)b * stride;
    const int64_t nb = nbytes[b];
    // the header is read only when the row holds one
    bool ok = nb >= 8 && nb <= stride && ((nb - 8) & 1) == 0 && (nb - 8) / 2 <= P;
    int bits = 1;
    if (ok) {
        const uint32_t magic = (uint32_t)in[0] | (uint32_t)in[1] << 8 | (uint32_t)in[2] << 16 | (uint32_t)in[3] << 24;
        bits = in[4];
        ok = magic == SUB_MAGIC && bits >= 1 && bits <= 4 && in[5] == 0 && in[6] == 0 && in[7] == 0;
    }
    if (!ok) bits = 1;   // (nothing is read through it then)
    // the number of pixels with a label other than 1 is what each plane must hold
    uint32_t mine = 0u;
    for (int p = threadIdx.x; p < P; p += INT_FRAME_THREADS) mine += labels[px0 + p] != (L)1 ? 1u : 0u;
    uint32_t n;
    (void)intensity_block_scan(mine, wsum, n);
    ok = ok && 2 * (int64_t)n == nb - 8;   // (workgroup-uniform)
    // every code of both planes is below L, or nothing of the frame is decoded (a code is an index into the table)
    const uint32_t Lc = 1u << (ok ? bits : 1);
    int bad = 0;
    if (ok)
        for (int64_t k = threadIdx.x; k < 2 * (int64_t)n; k += INT_FRAME_THREADS) bad |= in[8 + k] >= Lc ? 1 : 0;   // 8 + k < nb <= stride
    ok = !__syncthreads_or(bad) && ok;
    const double *ca = tables, *sa = tables + H, *cz = tables + 2 * H, *sz = tables + 2 * H + W;
    const double *step = tables + 2 * H + 2 * W + (int64_t)(bits - 1) * SUB_TABLE_CODES * 4;   // (bits is 1 .. 4 when ok, else 1)
    uint32_t running = 0u;
    for (int r0 = 0; r0 < P; r0 += INT_FRAME_THREADS * INT_PPT) {
        const int p0 = r0 + (int)threadIdx.x * INT_PPT;
        bool set[INT_PPT];
        uint32_t cnt = 0u;
#pragma unroll
        for (int k = 0; k < INT_PPT; k++) {
            set[k] = ok && p0 + k < P && labels[px0 + p0 + k] != (L)1;
            cnt += set[k] ? 1u : 0u;
        }
        uint32_t all = 0u, rank = 0u;
        if (ok) rank = running + intensity_block_scan(cnt, wsum, all);   // (workgroup-uniform branch)
#pragma unroll
        for (int k = 0; k < INT_PPT; k++) {
            if (p0 + k >= P) continue;
            float x = 0.0f, y = 0.0f, z = 0.0f;
            if (set[k]) {
                const uint32_t a = in[8 + rank], e = in[8 + n + rank];   // rank < n; both < Lc <= SUB_TABLE_CODES
                rank++;
                const int h = (p0 + k) / W, w = (p0 + k) - h * W;
                subpixel_turn_ray(ca, sa, cz, sz, step, h, w, a, e, (double)ri_rec[px0 + p0 + k], x, y, z);
            }
            float *o = points + 3 * (px0 + p0 + k);
            o[0] = x; o[1] = y; o[2] = z;
        }
        running += all;
    }
    if (threadIdx.x == 0) status[b] = ok ? RPCC_STREAM_OK : RPCC_STREAM_E_SUBPIXEL;
}
