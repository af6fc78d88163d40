// decode_tile.inc -- the body of decode_kernel and of decode_gated_kernel (codec_kernels.h), included into each with DECODE_GATED 0 / 1.
// Text, not a template or an inlined function: the ungated kernel then compiles to exactly the code it had before the gated one existed (as a
// function inlined into both, the same statements came out in another instruction order).
// Parameters in scope: seg, q16, model, tm, hist, salience, steps, P, M, KP, T, ri_rec, pc_rec -- and, gated, gate (StreamGate).
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float *smodel = reinterpret_cast<float *>(smem_raw);                 // [KP*4]
    uint32_t *segcnt = reinterpret_cast<uint32_t *>(smodel + 4 * KP);    // [16][KP+1]
    const int SEGP = KP + 1;
    uint32_t *soff = segcnt + 16 * SEGP;                                 // [KP] this tile's input offsets per label
    const int b = blockIdx.y, t = blockIdx.x, K = M + 2;
#if DECODE_GATED
    const int st = stream_final_status(gate, b);   // (the same for the whole workgroup)
    if (t == 0 && threadIdx.x == 0) gate.status[b] = st;
    if (st != RPCC_STREAM_OK) {
        uint8_t *sw = static_cast<uint8_t *>(gate.seg_w) + (int64_t)b * P;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int p = t * TILE + j * 256 + threadIdx.x;
            if (p >= P) continue;
            sw[p] = 0;
            ri_rec[(int64_t)b * P + p] = 0.0f;
            if (pc_rec) { float *o = pc_rec + ((int64_t)b * P + p) * 3; o[0] = 0.0f; o[1] = 0.0f; o[2] = 0.0f; }
        }
        return;
    }
    const int nrow = (int)(gate.payload_len[5 * (int64_t)b + 3] >> 4);   // model rows / salience entries the stream holds
    const int nsal = (int)gate.payload_len[5 * (int64_t)b];
#endif
    // per-frame bases (wave-uniform) + byte offsets; all loads of the tile are issued first (unconditional, clamped)
    seg += (int64_t)b * P;
    q16 += (int64_t)b * P;
    ri_rec += (int64_t)b * P;
    if (pc_rec) pc_rec += (int64_t)b * P * 3;
    int lab[4], rank[4], lraw[4];
    f32x3 ray[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint32_t p = (uint32_t)min(t * TILE + j * 256 + (int)threadIdx.x, P - 1);
        lraw[j] = ld_at(seg, p);
        ray[j] = ld_at(reinterpret_cast<const f32x3 *>(tm), p * 12u);
    }
#if DECODE_GATED
    for (int i = threadIdx.x; i < 4 * K; i += 256) smodel[i] = i < 4 * nrow ? model[(int64_t)b * K * 4 + i] : 0.0f;
#else
    for (int i = threadIdx.x; i < 4 * K; i += 256) smodel[i] = model[(int64_t)b * K * 4 + i];
#endif
    for (int i = threadIdx.x; i < K; i += 256) soff[i] = hist[((int64_t)b * T + t) * KP + i];
    for (int i = threadIdx.x; i < 16 * SEGP; i += 256) segcnt[i] = 0u;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int p = t * TILE + j * 256 + threadIdx.x;
        lab[j] = (p < P && lraw[j] != 1) ? lraw[j] : -1;
        rank[j] = segment_rank(j, lab[j], segcnt, SEGP);
    }
    segment_offsets(segcnt, SEGP, soff, K);
    int16_t qv[4];
#pragma unroll
    for (int j = 0; j < 4; j++)  // gather of the label-ordered integers (clamped: unused for label 1 / outside)
        qv[j] = ld_at(q16, (lab[j] >= 0 ? segment_slot(j, lab[j], rank[j], segcnt, SEGP) : 0u) * 2u);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int p = t * TILE + j * 256 + threadIdx.x;
        if (p >= P) continue;
        const int l = lraw[j];
        const float pr = intra_pred(smodel[4 * l], smodel[4 * l + 1], smodel[4 * l + 2], smodel[4 * l + 3], ray[j].x, ray[j].y, ray[j].z);
        float res = 0.0f;  // label 1 keeps the zero of np.zeros_like (compress_utils.py:115)
#if DECODE_GATED
        if (lab[j] >= 0) res = dequant(qv[j], steps.levels && l >= nsal ? steps.acc[0] : dequant_step(steps, salience, (int64_t)b * K + l));   // (level 0 of the zero padding)
#else
        if (lab[j] >= 0) res = dequant(qv[j], dequant_step(steps, salience, (int64_t)b * K + l));
#endif
        const float rec = pr + res;          // tools/decompress.py:104
        st_at(ri_rec, (uint32_t)p * 4u, rec);
        if (pc_rec) {
            f32x3 o;
            o.x = rec * ray[j].x; o.y = rec * ray[j].y; o.z = rec * ray[j].z;
            st_at(reinterpret_cast<f32x3 *>(pc_rec), (uint32_t)p * 12u, o);
        }
    }
