// codec_kernels.h -- contour codec (f1, f3) and the decoder's residual gather (f3); included by rpcc_hip.hip.
//
//   f1  extract_contour  ops/cpp_modules/src/cpp_modules.cpp:521-558  +  np.packbits / uint16 casts of
//       compress_point_cloud (utils/compress_utils.py:156-160)
//   f3  recover_map      cpp_modules.cpp:561-593;  dequantize_residual  utils/compress_utils.py:114-132;
//       range_image_rec = pred + residual, range_image_to_point_cloud  (tools/decompress.py:88-112)
#pragma once

// ------------------------------------------------------------------------------------------------
// f1: contour bit of pixel (h,w) = (w == 0) || seg[h,w] != seg[h,w-1]; idx_sequence = labels at the
// contour positions in row-major order (uint16); contour_map = np.packbits (first pixel = MSB).
// Pass 1 counts contour bits per 1024-pixel tile, pass 2 turns the counts into offsets (one workgroup
// per frame), pass 3 writes the packed bits and scatters the labels.
// ------------------------------------------------------------------------------------------------
// (L: the label type -- uint8_t, or uint16_t for cluster_num above RPCC_MAX_CLUSTERS, wide_kernels.h)
template <class L>
__device__ __forceinline__ bool contour_bit(const L *__restrict__ seg, int p, int W) {
    const int col = p % W;
    return col == 0 || seg[p] != seg[p - 1];
}

template <class L>
__global__ __launch_bounds__(256) void contour_count_kernel(const L *__restrict__ seg, int P, int W, int T,
                                                            uint32_t *__restrict__ tile_cnt) {
    __shared__ int s[4];
    const int b = blockIdx.y, t = blockIdx.x;
    const L *sg = seg + (int64_t)b * P;
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < TILE / 256; j++) {
        const int p = t * TILE + j * 256 + threadIdx.x;
        const bool c = p < P && contour_bit(sg, min(p, P - 1), W);
        cnt += __popcll(__ballot(c));
    }
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) tile_cnt[(int64_t)b * T + t] = (uint32_t)(s[0] + s[1] + s[2] + s[3]);
}

// exclusive scan of the per-tile counts of one frame (T <= 4096 handled in chunks of 256) -> the frame's total, in every thread
__device__ __forceinline__ uint32_t tile_scan_body(uint32_t *__restrict__ c, int T, uint32_t *sh) {
    uint32_t run = 0;
    for (int base = 0; base < T; base += 256) {
        const int i = base + threadIdx.x;
        const uint32_t v = i < T ? c[i] : 0u;
        sh[threadIdx.x] = v;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {  // Hillis-Steele inclusive scan
            const uint32_t add = (int)threadIdx.x >= o ? sh[threadIdx.x - o] : 0u;
            __syncthreads();
            sh[threadIdx.x] += add;
            __syncthreads();
        }
        if (i < T) c[i] = run + sh[threadIdx.x] - v;
        run += sh[255];
        __syncthreads();
    }
    return run;
}
// ... of every frame of a batch, total -> nseq
__global__ __launch_bounds__(256) void tile_scan_kernel(uint32_t *__restrict__ tile_cnt, int T, int32_t *__restrict__ total) {
    __shared__ uint32_t sh[256];
    const int b = blockIdx.x;
    const uint32_t run = tile_scan_body(tile_cnt + (int64_t)b * T, T, sh);
    if (threadIdx.x == 0 && total) total[b] = (int32_t)run;
}

template <class L>
__global__ __launch_bounds__(256) void contour_write_kernel(const L *__restrict__ seg, int P, int W, int T,
                                                            const uint32_t *__restrict__ tile_off,
                                                            uint8_t *__restrict__ bits, uint16_t *__restrict__ seq) {
    __shared__ uint32_t segcnt[16];
    const int b = blockIdx.y, t = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const L *sg = seg + (int64_t)b * P;
    const int nbytes = (P + 7) >> 3;
    uint8_t *ob = bits + (int64_t)b * nbytes;
    uint16_t *os = seq + (int64_t)b * P;
    bool c[TILE / 256];
    unsigned long long m[TILE / 256];
#pragma unroll
    for (int j = 0; j < TILE / 256; j++) {
        const int p = t * TILE + j * 256 + threadIdx.x;
        c[j] = p < P && contour_bit(sg, min(p, P - 1), W);
        m[j] = __ballot(c[j]);
        if (lane == 0) segcnt[j * 4 + wave] = (uint32_t)__popcll(m[j]);
        // 64 pixels -> 8 bytes, pixel 8k+i of the segment is bit (7-i) of byte k
        if (lane < 8) {
            const int byte_idx = ((t * TILE + j * 256 + wave * 64) >> 3) + lane;
            if (byte_idx < nbytes) {
                const uint32_t v = (uint32_t)((m[j] >> (8 * lane)) & 0xFFull);
                ob[byte_idx] = (uint8_t)(__brev(v) >> 24);
            }
        }
    }
    __syncthreads();
    uint32_t run = tile_off[(int64_t)b * T + t];
#pragma unroll
    for (int j = 0; j < TILE / 256; j++) {
#pragma unroll
        for (int w = 0; w < 4; w++) {
            const uint32_t n = segcnt[j * 4 + w];
            if (w == wave && c[j]) {
                const int p = t * TILE + j * 256 + threadIdx.x;
                os[run + __popcll(m[j] & ((1ull << lane) - 1ull))] = (uint16_t)sg[p];
            }
            run += n;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// f3, batched streams (rpcc_decompress_batch): the checks tools/decompress.py:decode_frame makes on the host before it lets the kernels index
// with a stream's contents, as a status per frame (RPCC_STREAM_*, rpcc_hip.h: the first check that fails, in decode_frame's order).
// Checks 1..4 follow from the lengths and the entropy statuses alone (stream_length_status: every workgroup evaluates them for itself);
// a frame that fails one is not read at all.  stream_check_kernel: per frame x tile, the popcount of the tile's contour bits (the pad bits of
// the last byte do not count) -- the tile counts recover_map scans --, the largest idx entry of the tile's share of the stream's
// entries and (tile 0) the largest salience level.  stream_status_kernel: per frame, the scan of the tile counts, whose total is the
// popcount, and the status of checks 1..7.  Check 8 needs the label map: decode_body<true>.
// Nothing past a payload's stated length is read.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int stream_length_status(const int64_t *__restrict__ len, const int32_t *__restrict__ est, bool nonuniform, int P, int K) {
    for (int c = nonuniform ? 0 : 1; c < 5; c++)
        if (est[c] != 0) return RPCC_STREAM_E_ENTROPY;
    const int64_t plane = len[3];
    if (plane < 0 || (plane & 15) != 0 || (plane >> 4) > K) return RPCC_STREAM_E_PLANE;
    if (len[1] != (int64_t)((P + 7) >> 3)) return RPCC_STREAM_E_CONTOUR;
    if (len[2] < 0 || (len[2] & 1) != 0 || len[4] < 0 || (len[4] & 1) != 0) return RPCC_STREAM_E_WIDTH;
    return RPCC_STREAM_OK;
}
__global__ __launch_bounds__(256) void stream_check_kernel(const uint8_t *__restrict__ bits, const uint16_t *__restrict__ seq,
                                                           const uint8_t *__restrict__ salience, const int64_t *__restrict__ payload_len,
                                                           const int32_t *__restrict__ entropy_status, int nonuniform, int P, int K, int T,
                                                           uint32_t *__restrict__ tile_cnt, uint32_t *__restrict__ tile_max,
                                                           uint32_t *__restrict__ sal_max) {
    __shared__ uint32_t s[3][4];
    const int b = blockIdx.y, t = blockIdx.x;
    const int64_t *len = payload_len + 5 * (int64_t)b;
    const bool sound = stream_length_status(len, entropy_status + 5 * (int64_t)b, nonuniform != 0, P, K) == RPCC_STREAM_OK;
    uint32_t cnt = 0u, imax = 0u, smax = 0u;
    if (sound) {
        const int nbytes = (P + 7) >> 3;
        // a tile = 1024 pixels = 128 bytes; threads 0..127 take one byte each
        const int byte_idx = t * (TILE / 8) + threadIdx.x;
        if (threadIdx.x < TILE / 8 && byte_idx < nbytes) {
            uint32_t v = bits[(int64_t)b * nbytes + byte_idx];
            const int valid = P - byte_idx * 8;  // pixels of this byte inside the image
            if (valid < 8) v &= 0xFFu << (8 - valid);
            cnt = (uint32_t)__popc(v);
        }
        const int nidx = (int)min(len[2] >> 1, (int64_t)P);   // (more entries than pixels: refused by the count, whatever they hold)
#pragma unroll
        for (int j = 0; j < TILE / 256; j++) {
            const int p = t * TILE + j * 256 + threadIdx.x;
            if (p < nidx) imax = max(imax, (uint32_t)seq[(int64_t)b * P + p]);
        }
        if (nonuniform && t == 0) {
            const int nsal = (int)min(max(len[0], (int64_t)0), (int64_t)K);
            for (int i = threadIdx.x; i < nsal; i += 256) smax = max(smax, (uint32_t)salience[(int64_t)b * K + i]);
        }
    }
    cnt = dpp_sum_u32(cnt);
    imax = dpp_max_u32(imax);
    smax = dpp_max_u32(smax);
    if ((threadIdx.x & 63) == 0) { s[0][threadIdx.x >> 6] = cnt; s[1][threadIdx.x >> 6] = imax; s[2][threadIdx.x >> 6] = smax; }
    __syncthreads();
    if (threadIdx.x == 0) {
        tile_cnt[(int64_t)b * T + t] = s[0][0] + s[0][1] + s[0][2] + s[0][3];
        tile_max[(int64_t)b * T + t] = max(max(s[1][0], s[1][1]), max(s[1][2], s[1][3]));
        if (t == 0) sal_max[b] = max(max(s[2][0], s[2][1]), max(s[2][2], s[2][3]));
    }
}
__global__ __launch_bounds__(256) void stream_status_kernel(uint32_t *__restrict__ tile_cnt, const uint32_t *__restrict__ tile_max,
                                                            const uint32_t *__restrict__ sal_max, const int64_t *__restrict__ payload_len,
                                                            const int32_t *__restrict__ entropy_status, int levels, int P, int K, int T,
                                                            int32_t *__restrict__ pre_status) {
    __shared__ uint32_t sh[256];
    __shared__ uint32_t smx[4];
    const int b = blockIdx.x;
    const uint32_t nbits = tile_scan_body(tile_cnt + (int64_t)b * T, T, sh);
    uint32_t imax = 0u;
    for (int i = threadIdx.x; i < T; i += 256) imax = max(imax, tile_max[(int64_t)b * T + i]);
    imax = dpp_max_u32(imax);
    if ((threadIdx.x & 63) == 0) smx[threadIdx.x >> 6] = imax;
    __syncthreads();
    if (threadIdx.x != 0) return;
    imax = max(max(smx[0], smx[1]), max(smx[2], smx[3]));
    const int64_t *len = payload_len + 5 * (int64_t)b;
    int st = stream_length_status(len, entropy_status + 5 * (int64_t)b, levels != 0, P, K);
    if (st == RPCC_STREAM_OK) {
        const int64_t nidx = len[2] >> 1, rows = len[3] >> 4;
        if (nidx != (int64_t)nbits) st = RPCC_STREAM_E_NSEQ;
        else if (nidx > 0 && (int64_t)imax >= rows) st = RPCC_STREAM_E_LABEL;
        else if (levels != 0 && (len[0] > K || len[0] < rows || (len[0] > 0 && (int)sal_max[b] >= levels))) st = RPCC_STREAM_E_SALIENCE;
    }
    pre_status[b] = st;
}

// f3: recover_map.  Label of pixel p = seq[(number of contour bits at positions <= p) - 1].
__global__ __launch_bounds__(256) void contour_bits_count_kernel(const uint8_t *__restrict__ bits, int P, int T,
                                                                 uint32_t *__restrict__ tile_cnt) {
    __shared__ int s[4];
    const int b = blockIdx.y, t = blockIdx.x;
    const int nbytes = (P + 7) >> 3;
    const uint8_t *ib = bits + (int64_t)b * nbytes;
    // a tile = 1024 pixels = 128 bytes; threads 0..127 take one byte each
    int cnt = 0;
    if (threadIdx.x < TILE / 8) {
        const int byte_idx = t * (TILE / 8) + threadIdx.x;
        if (byte_idx < nbytes) {
            uint32_t v = ib[byte_idx];
            const int valid = P - byte_idx * 8;  // pixels of this byte inside the image
            if (valid < 8) v &= 0xFFu << (8 - valid);
            cnt = __popc(v);
        }
    }
    cnt = (int)dpp_sum_u32((uint32_t)cnt);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) tile_cnt[(int64_t)b * T + t] = (uint32_t)(s[0] + s[1] + s[2] + s[3]);
}

// GATED (rpcc_decompress_batch): gate[b] != 0 -- a frame the stream check refused: its workgroups read nothing and write the zeros themselves.
template <class L, bool GATED>
__device__ __forceinline__ void recover_map_body(const uint8_t *__restrict__ bits, const uint16_t *__restrict__ seq,
                                                 int P, int T, const uint32_t *__restrict__ tile_off, const int32_t *__restrict__ gate,
                                                 L *__restrict__ seg) {
    __shared__ uint32_t segcnt[16];
    const int b = blockIdx.y, t = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if constexpr (GATED) {
        if (gate[b] != 0) {   // (the same for the whole workgroup)
#pragma unroll
            for (int j = 0; j < TILE / 256; j++) {
                const int p = t * TILE + j * 256 + threadIdx.x;
                if (p < P) seg[(int64_t)b * P + p] = (L)0;
            }
            return;
        }
    }
    const int nbytes = (P + 7) >> 3;
    const uint8_t *ib = bits + (int64_t)b * nbytes;
    const uint16_t *is = seq + (int64_t)b * P;
    bool c[TILE / 256];
    unsigned long long m[TILE / 256];
#pragma unroll
    for (int j = 0; j < TILE / 256; j++) {
        const int p = t * TILE + j * 256 + threadIdx.x;
        const int pc = min(p, P - 1);
        c[j] = p < P && ((ib[pc >> 3] >> (7 - (pc & 7))) & 1);
        m[j] = __ballot(c[j]);
        if (lane == 0) segcnt[j * 4 + wave] = (uint32_t)__popcll(m[j]);
    }
    __syncthreads();
    uint32_t run = tile_off[(int64_t)b * T + t];
#pragma unroll
    for (int j = 0; j < TILE / 256; j++) {
#pragma unroll
        for (int w = 0; w < 4; w++) {
            if (w == wave) {
                const int p = t * TILE + j * 256 + threadIdx.x;
                // inclusive count of contour bits up to this pixel
                const uint32_t k = run + (uint32_t)__popcll(m[j] & ((2ull << lane) - 1ull));
                if (p < P) seg[(int64_t)b * P + p] = (L)(k ? is[k - 1] : 0);
            }
            run += segcnt[j * 4 + w];
        }
    }
}
template <class L>
__global__ __launch_bounds__(256) void recover_map_kernel(const uint8_t *__restrict__ bits, const uint16_t *__restrict__ seq,
                                                          int P, int T, const uint32_t *__restrict__ tile_off,
                                                          L *__restrict__ seg) {
    recover_map_body<L, false>(bits, seq, P, T, tile_off, nullptr, seg);
}
template <class L>
__global__ __launch_bounds__(256) void recover_map_gated_kernel(const uint8_t *__restrict__ bits, const uint16_t *__restrict__ seq,
                                                                int P, int T, const uint32_t *__restrict__ tile_off,
                                                                const int32_t *__restrict__ gate, L *__restrict__ seg) {
    recover_map_body<L, true>(bits, seq, P, T, tile_off, gate, seg);
}

// ------------------------------------------------------------------------------------------------
// f3: decoder body.  For every pixel: pred (intra_pred), residual = dequant of the integer read from the
// label-ordered stream at its slot (segment_slot: the inverse of the encoder's ordered scatter),
// rec = pred + residual (fp32), optional point cloud rec * tm.
// steps (DecodeSteps, ref_rules.h): one double (uniform) or per-label through salience (non-uniform).
// ------------------------------------------------------------------------------------------------
// Gated form (rpcc_decompress_batch, StreamGate below; the body of both kernels: decode_tile.inc): the frame's status is settled here -- the stream check's, or E_RESIDUAL when the stream's
// residual count is not the label map's -- and a refused frame's workgroups read nothing and write the zeros themselves, the label map's included.
// Rows of `model` / entries of `salience` past the stream's own count are read as zero (they may hold anything).
struct StreamGate {
    const int32_t *pre;        // [B] status after the stream check (checks 1..7)
    const int32_t *nnz;        // [B] pixels whose recovered label is not 1
    const int64_t *payload_len;// [B,5]
    int32_t *status;           // [B] out
    void *seg_w;               // the label map, to zero a frame refused here
};
__device__ __forceinline__ int stream_final_status(const StreamGate &g, int b) {
    const int pre = g.pre[b];
    return pre ? pre : ((g.payload_len[5 * (int64_t)b + 4] >> 1) != (int64_t)g.nnz[b] ? RPCC_STREAM_E_RESIDUAL : RPCC_STREAM_OK);
}
__global__ __launch_bounds__(256) void decode_kernel(const uint8_t *__restrict__ seg, const int16_t *__restrict__ q16,
                                                     const float *__restrict__ model, const float *__restrict__ tm,
                                                     const uint32_t *__restrict__ hist, const uint8_t *__restrict__ salience,
                                                     DecodeSteps steps, int P, int M, int KP, int T,
                                                     float *__restrict__ ri_rec, float *__restrict__ pc_rec) {
#define DECODE_GATED 0
#include "decode_tile.inc"
#undef DECODE_GATED
}
__global__ __launch_bounds__(256) void decode_gated_kernel(const uint8_t *__restrict__ seg, const int16_t *__restrict__ q16,
                                                           const float *__restrict__ model, const float *__restrict__ tm,
                                                           const uint32_t *__restrict__ hist, const uint8_t *__restrict__ salience,
                                                           DecodeSteps steps, int P, int M, int KP, int T,
                                                           float *__restrict__ ri_rec, float *__restrict__ pc_rec, StreamGate gate) {
#define DECODE_GATED 1
#include "decode_tile.inc"
#undef DECODE_GATED
}
// its LDS: smodel f32 [KP*4] | the segments'
static inline size_t decode_lds_bytes(int KP) { return (size_t)KP * 4 * 4 + segment_lds_bytes(KP); }

// a3 as its own entry: pc = ri[...,None] * transform_map  (dataset/transformer.py:94-101)
__global__ __launch_bounds__(256) void backproject_kernel(const float *__restrict__ ri, const float *__restrict__ tm, int P,
                                                          float *__restrict__ pc) {
    const int b = blockIdx.y;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < P) {
        const float r = ri[(int64_t)b * P + p];
        float *o = pc + ((int64_t)b * P + p) * 3;
        o[0] = r * tm[3 * p]; o[1] = r * tm[3 * p + 1]; o[2] = r * tm[3 * p + 2];
    }
}

// f2: the batch's residual stream as the container holds it -- the frames' label-ordered int16 runs back to back
// (`residual_quantized` of compress_point_cloud, utils/compress_utils.py:142,160: one array of nnz entries per
// frame).  packed[prefix(b) + i] = q16[b][i] for i < nnz[b], prefix(b) = nnz[0] + ... + nnz[b-1] computed on the
// device, so neither the D2H copy nor the RCCL gather of a rank's payloads moves the B*P padded array.
// One workgroup copies PACK_EPW entries: 2-byte accesses, lane-consecutive (the destination has no alignment),
// PACK_EPT loads in flight per lane.
#define PACK_EPT 8
#define PACK_EPW (256 * PACK_EPT)
__global__ __launch_bounds__(256) void pack_payload_kernel(const int16_t *__restrict__ q16, const int32_t *__restrict__ nnz,
                                                           int P, int64_t capacity, int16_t *__restrict__ packed,
                                                           int64_t *__restrict__ total) {
    const int b = blockIdx.y, B = gridDim.y;
    const int n = min(max(nnz[b], 0), P);
    const int i0 = blockIdx.x * PACK_EPW;
    const bool last = b == B - 1 && blockIdx.x == 0 && total != nullptr;
    if (i0 >= n && !last) return;
    // prefix over the earlier frames: every wavefront computes it for itself (B is a few hundred values)
    const int lane = threadIdx.x & 63;
    int64_t pre = 0;
    for (int j = lane; j < b; j += 64) pre += min(max(nnz[j], 0), P);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) pre += __shfl_xor(pre, o, RPCC_WAVE);
    if (last && threadIdx.x == 0) *total = pre + n;
    const int16_t *src = q16 + (int64_t)b * P;
    int16_t v[PACK_EPT];
#pragma unroll
    for (int k = 0; k < PACK_EPT; k++) {
        const int i = i0 + k * 256 + (int)threadIdx.x;
        v[k] = src[min(i, P - 1)];
    }
#pragma unroll
    for (int k = 0; k < PACK_EPT; k++) {
        const int i = i0 + k * 256 + (int)threadIdx.x;
        if (i < n && pre + i < capacity) packed[pre + i] = v[k];
    }
}
