// labels_kernels.h -- the batch entered with a caller's label map (rpcc_compress_batch_labels): the label intake and
// the pass that clears what a refused frame left.  Included by rpcc_hip.hip behind the histogram (hist_aggregate, TILE) it feeds.
#pragma once

// Label intake.  One workgroup per 1024-pixel tile (the histogram's tiling), a lane owns four consecutive pixels: one 16-byte load of the
// int32 labels and -- SUMS, the point model -- one of the ranges, both issued before anything is used; 256 threads, no LDS beyond the
// histogram's tables (the footprint lesson of DESIGN.md section 8).  It
//   * narrows the labels to L (one 4- or 8-byte store per lane in the VEC form),
//   * notes in tile_bad[b][t] whether a label of the tile lies outside 0 .. lim, lim = max_label[b] -- or nothing at all when max_label[b]
//     is itself outside 0 .. M + 1 (RPCC_SEG_CAPPED is negative).  Such a label is stored as 1 (an empty pixel), so that nothing behind
//     this kernel indexes with it; labels_refuse_kernel turns the frame's rows into zeros at the end,
//   * leaves what model_hist_kernel leaves: hist[b][t][.] and, with SUMS, the labels' range sums and the frame's flag (hist_aggregate), so the
//     narrow map is not read again for them.  sums / flags are zero at entry (the entry's memset); tile_bad and hist are plain stores,
//   * clears the key-point counters of the non-uniform framework (zero: a grid-stride loop, as batch_init does it).
// VEC: P % 4 == 0 and labels, seg (and ri) aligned for the quad accesses.
template <bool VEC, class L, bool SUMS>
__global__ __launch_bounds__(256) void labels_in_kernel(const int32_t *__restrict__ labels, const int32_t *__restrict__ max_label,
                                                        const float *__restrict__ ri, int P, int M, int KP, int T, L *__restrict__ seg,
                                                        int64_t *__restrict__ sums, int32_t *__restrict__ flags, uint32_t *__restrict__ hist,
                                                        int32_t *__restrict__ tile_bad, ZeroRange zero) {
    const int b = blockIdx.y, t = blockIdx.x;
    const int32_t *lab_b = labels + (int64_t)b * P;
    const float *ri_b = SUMS ? ri + (int64_t)b * P : nullptr;
    L *seg_b = seg + (int64_t)b * P;
    const int p0 = t * TILE + 4 * (int)threadIdx.x;
    const int nval = min(max(P - p0, 0), 4);
    int lab[4];
    uint32_t rb[4];
    // all loads first (unconditional, clamped)
    if (VEC) {
        const uint32_t q = (uint32_t)(nval > 0 ? p0 : 0);
        const int4 l4 = ld_at(reinterpret_cast<const int4 *>(lab_b), q * 4u);
        lab[0] = l4.x; lab[1] = l4.y; lab[2] = l4.z; lab[3] = l4.w;
        if constexpr (SUMS) {
            const uint4 r4 = ld_at(reinterpret_cast<const uint4 *>(ri_b), q * 4u);
            rb[0] = r4.x; rb[1] = r4.y; rb[2] = r4.z; rb[3] = r4.w;
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const uint32_t gp = (uint32_t)min(p0 + e, P - 1);
            lab[e] = ld_at(lab_b, gp * 4u);
            if constexpr (SUMS) rb[e] = f2u(ld_at(ri_b, gp * 4u));
        }
    }
    const int mx = max_label[b];
    const int lim = (mx < 0 || mx > M + 1) ? -1 : mx;   // -1: every label of the frame is refused
    {
        const int nthr = (int)(gridDim.x * gridDim.y) * 256, me = (b * (int)gridDim.x + t) * 256 + (int)threadIdx.x;
        for (int i = me; i < zero.n; i += nthr) zero.p[i] = 0u;
    }
    bool bad = false;
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const bool ok = lab[e] >= 0 && lab[e] <= lim;
        bad |= e < nval && !ok;
        lab[e] = ok ? lab[e] : 1;
    }
    if (VEC) {
        if (nval > 0) {
            if constexpr (sizeof(L) == 1)
                st_at(reinterpret_cast<uint32_t *>(seg_b), (uint32_t)p0, (uint32_t)lab[0] | ((uint32_t)lab[1] << 8) | ((uint32_t)lab[2] << 16) | ((uint32_t)lab[3] << 24));
            else
                st_at(reinterpret_cast<uint2 *>(seg_b), (uint32_t)p0 * 2u, make_uint2((uint32_t)lab[0] | ((uint32_t)lab[1] << 16), (uint32_t)lab[2] | ((uint32_t)lab[3] << 16)));
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4; e++)
            if (e < nval) st_at(seg_b, (uint32_t)(p0 + e) * (uint32_t)sizeof(L), (L)lab[e]);
    }
    const int any_bad = __syncthreads_or(bad ? 1 : 0);
    if (threadIdx.x == 0) tile_bad[(int64_t)b * T + t] = any_bad;
    hist_aggregate<SUMS>(lab, rb, nval, KP, T, sums, flags, hist, b, t);
}

// The frames' statuses, and zeros in every output row of a refused frame.  Same grid as the intake (T x B workgroups of 256 threads); a
// workgroup of a sound frame reads the frame's T tile notes and leaves.  seg, q16 (all P entries) and key_point_map by tile; model, counts,
// salience and nnz by the frame's first workgroup.  salience / key_point_map: NULL in the uniform framework.
template <class L>
__global__ __launch_bounds__(256) void labels_refuse_kernel(const int32_t *__restrict__ max_label, const int32_t *__restrict__ tile_bad, int P, int M, int T,
                                                            int32_t *__restrict__ status, L *__restrict__ seg, float *__restrict__ model,
                                                            int32_t *__restrict__ counts, int16_t *__restrict__ q16, int32_t *__restrict__ nnz,
                                                            uint8_t *__restrict__ salience, uint8_t *__restrict__ key_point_map) {
    const int b = blockIdx.y, t = blockIdx.x, K = M + 2;
    int bad = 0;
    for (int i = threadIdx.x; i < T; i += 256) bad |= tile_bad[(int64_t)b * T + i];
    bad = __syncthreads_or(bad);
    const int mx = max_label[b];
    const int st = mx == RPCC_LABELS_CAPPED ? RPCC_LABELS_E_CAPPED : (mx < 0 || mx > M + 1 || bad) ? RPCC_LABELS_E_RANGE : RPCC_LABELS_OK;
    if (t == 0 && threadIdx.x == 0) status[b] = st;
    if (st == RPCC_LABELS_OK) return;
    const int p0 = t * TILE, p1 = min(P, p0 + TILE);
    for (int p = p0 + (int)threadIdx.x; p < p1; p += 256) {
        seg[(int64_t)b * P + p] = (L)0;
        q16[(int64_t)b * P + p] = (int16_t)0;
        if (key_point_map) key_point_map[(int64_t)b * P + p] = (uint8_t)0;
    }
    if (t == 0) {
        for (int k = threadIdx.x; k < K; k += 256) {
            float *row = model + ((int64_t)b * K + k) * 4;
            row[0] = row[1] = row[2] = row[3] = 0.0f;
            counts[(int64_t)b * K + k] = 0;
            if (salience) salience[(int64_t)b * K + k] = (uint8_t)0;
        }
        if (threadIdx.x == 0) nnz[b] = 0;
    }
}
