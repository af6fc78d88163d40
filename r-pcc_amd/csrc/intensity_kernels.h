// Lidar intensity through the codec (include/rpcc_hip.h "intensity"; the specification is stated once, in tests/intensity_ref.py).
// Included from rpcc_hip.hip after the projection: the pixel of a point comes from project_point_fast / project_point, the two
// functions that produced ri, so it cannot differ from the pixel the depth was written to.
//
//   owner pass      every point once: a point whose depth bits equal ri at its pixel does atomicMin(owner[pix], position in its frame).
//                   A depth-0 point records atomicMax(lastz[pix], position + 1) and flags its frame; flagged frames are redone
//                   restricted to positions after lastz (the MODE 0 / 1 / 2 structure of project_kernel, the lastz pass folded into
//                   the first one).  Minima and maxima only: the result does not depend on scheduling.
//   pack pass       one workgroup per frame, raster order: non-empty mask from ri, exclusive rank by a workgroup scan, the owner's
//                   fourth float quantised to payload[8 + rank]; header, nbytes, orphans, optionally the u8 image and the owners' floats.
//   decode pass     one workgroup per frame: the header and the count of labels != 1 are checked first, then the same scan
//                   spreads payload[8 + rank] / scale over the pixels.  A refused frame is written as zeros.
#define INT_NO_OWNER 0x7FFFFFFF
#define INT_THREADS 256
#define INT_MAGIC 0x31495052u   // "RPI1", little-endian
#define INT_FRAME_THREADS 1024
#define INT_PPT 4               // pixels per thread and round of the per-frame kernels (consecutive: raster order inside a thread)

struct IntensityLayout { int32_t *owner, *lastz, *flags; size_t bytes; };
static IntensityLayout intensity_layout(void *scratch, int B, int P) {
    Carve c(scratch);
    IntensityLayout l;
    l.owner = c.take<int32_t>((size_t)B * P * 4, 4);
    l.lastz = c.take<int32_t>((size_t)B * P * 4, 4);
    l.flags = c.take<int32_t>((size_t)(B + 1) * 4, 4);   // per frame: holds a depth-0 point; [B]: any frame does
    l.bytes = round_up(c.bytes(), 256);
    return l;
}

__global__ __launch_bounds__(256) void intensity_fill_kernel(int32_t *__restrict__ owner, int32_t *__restrict__ lastz, int32_t *__restrict__ flags,
                                                             int64_t n, int B, bool fixup, int P) {
    if (fixup) {   // owners of the flagged frames again (lastz is kept)
        if (flags[B] == 0) return;
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
            if (flags[i / P] != 0) owner[i] = INT_NO_OWNER;
        return;
    }
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        owner[i] = INT_NO_OWNER;
        lastz[i] = 0;
    }
    if (blockIdx.x == 0)
        for (int b = threadIdx.x; b <= B; b += blockDim.x) flags[b] = 0;
}

// a point of finite depth whose pixel is known.  FIXUP: only positions after the pixel's last depth-0 point compete.
template <bool FIXUP>
__device__ __forceinline__ void intensity_claim(int64_t at, int32_t idx, float depth, const uint32_t *__restrict__ ri, int32_t *__restrict__ owner,
                                                const int32_t *__restrict__ lastz) {
    if (f2u(depth) != ri[at]) return;
    if (FIXUP && idx + 1 <= lastz[at]) return;
    atomicMin(&owner[at], idx);
}

template <bool FIXUP>
__device__ __forceinline__ void intensity_exact_point(const float4 *__restrict__ rows, const int64_t *__restrict__ offs, int B, const rpcc_geom g,
                                                      int64_t i, const uint32_t *__restrict__ ri, int32_t *__restrict__ owner,
                                                      int32_t *__restrict__ lastz, int32_t *__restrict__ flags) {
    const float4 p = rows[i];
    const RowCol rc = project_point(p.x, p.y, p.z, g);
    if (!(fabsf(rc.depth) <= 3.402823466e+38f)) return;   // NaN / inf depth: skipped, as rpcc_project skips it
    const int b = find_frame(offs, B, i);
    if (FIXUP && flags[b] == 0) return;
    const int64_t at = (int64_t)b * g.H * g.W + rc.pix;
    const int32_t idx = (int32_t)(i - offs[b]);
    if (rc.depth == 0.0f) {
        if (!FIXUP) { flags[b] = 1; flags[B] = 1; atomicMax(&lastz[at], idx + 1); }
        return;
    }
    intensity_claim<FIXUP>(at, idx, rc.depth, ri, owner, lastz);
}

// Grid-stride over the points in rounds of one per thread; a point the screened pixel is not certain for waits in an LDS queue that
// full workgroups drain through the exact sequence (project_pix_kernel's scheme, without its records).
template <bool FIXUP>
__global__ __launch_bounds__(INT_THREADS) void intensity_owner_kernel(const float4 *__restrict__ rows, const int64_t *__restrict__ offs, int64_t total,
                                                                       int B, rpcc_geom g, PixFastCfg cfg, const uint32_t *__restrict__ ri,
                                                                       int32_t *__restrict__ owner, int32_t *__restrict__ lastz,
                                                                       int32_t *__restrict__ flags) {
    __shared__ uint32_t queue[2 * INT_THREADS];
    __shared__ uint32_t qn;
    if (FIXUP && flags[B] == 0) return;   // no frame of this batch holds a depth-0 point
    if (threadIdx.x == 0) qn = 0u;
    __syncthreads();
    const int64_t P = (int64_t)g.H * g.W;
    const int64_t lo = offs[0], hi = min(offs[B], total);   // rows outside the frames belong to nobody
    const int lane = threadIdx.x & 63;
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int64_t c = (int64_t)blockIdx.x * INT_THREADS; c < total; c += (int64_t)gridDim.x * INT_THREADS) {   // (workgroup-uniform)
        const int64_t i = c + threadIdx.x;
        bool in = i >= lo && i < hi;
        const int64_t ic = in ? i : 0;   // a row that exists (total > 0 here)
        const float4 p = rows[ic];
        int b = __builtin_amdgcn_readfirstlane(find_frame(offs, B, __shfl(ic, 0, 64)));   // one search per wavefront; lanes past that frame search again
        if (ic < offs[b] || ic >= offs[b + 1]) b = find_frame(offs, B, ic);
        if (FIXUP) in = in && flags[b] != 0;
        int pix;
        const bool fast = project_point_fast(p.x, p.y, p.z, g, cfg, pix) && cfg.on && in;
        const float depth = sqrt_rn_normal(p.x * p.x + p.y * p.y + p.z * p.z);   // == sqrtf, finite and not 0 when `fast` (as project_pix_kernel)
        if (fast) intensity_claim<FIXUP>((int64_t)b * P + pix, (int32_t)(ic - offs[b]), depth, ri, owner, lastz);
        const bool slow = in && !fast;
        const unsigned long long sm = __ballot(slow);
        if (sm) {
            const int leader = (int)__ffsll((long long)sm) - 1;
            uint32_t q0 = 0u;
            if (lane == leader) q0 = atomicAdd(&qn, (uint32_t)__popcll(sm));
            q0 = (uint32_t)__builtin_amdgcn_readlane((int)q0, leader);
            if (slow) queue[q0 + __popcll(sm & lt)] = (uint32_t)i;   // (total < 2^31)
        }
        __syncthreads();
        const uint32_t n = qn;
        if (n >= INT_THREADS) {   // (workgroup-uniform; n < 2 * INT_THREADS)
            intensity_exact_point<FIXUP>(rows, offs, B, g, (int64_t)queue[n - INT_THREADS + threadIdx.x], ri, owner, lastz, flags);
            __syncthreads();
            if (threadIdx.x == 0) qn = n - INT_THREADS;
        }
        __syncthreads();
    }
    const uint32_t n = qn;
    if (threadIdx.x < n) intensity_exact_point<FIXUP>(rows, offs, B, g, (int64_t)queue[threadIdx.x], ri, owner, lastz, flags);
}

// q of tests/intensity_ref.py: one fp32 multiply, round half to even, 0 unless r >= 0 (NaN, negatives), 255 above 255 (+inf)
__device__ __forceinline__ uint32_t intensity_quantise(float w, float scale) {
    const float r = rintf(w * scale);
    if (!(r >= 0.0f)) return 0u;
    if (r > 255.0f) return 255u;
    return (uint32_t)r;
}

// exclusive offset of this thread's count inside the workgroup, and the workgroup's total (INT_FRAME_THREADS threads, all active)
__device__ __forceinline__ uint32_t intensity_block_scan(uint32_t cnt, uint32_t *wsum, uint32_t &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t incl = dpp_scan_incl_u32(cnt);
    __syncthreads();   // (wsum of the round before has been read)
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t before = 0u, all = 0u;
#pragma unroll
    for (int w = 0; w < INT_FRAME_THREADS / 64; w++) {
        const uint32_t s = wsum[w];
        before += w < wave ? s : 0u;
        all += s;
    }
    total = all;
    return before + incl - cnt;
}

__global__ __launch_bounds__(INT_FRAME_THREADS) void intensity_pack_kernel(const float *__restrict__ rows, const int64_t *__restrict__ offs, int64_t total,
                                                                            int P, const float *__restrict__ ri, const int32_t *__restrict__ owner,
                                                                            float scale, uint8_t *__restrict__ payload, int64_t stride,
                                                                            int32_t *__restrict__ nbytes, uint8_t *__restrict__ image,
                                                                            float *__restrict__ owner_w, int32_t *__restrict__ orphans) {
    __shared__ uint32_t wsum[INT_FRAME_THREADS / 64];
    __shared__ uint32_t lost;
    const int b = blockIdx.x;
    if (threadIdx.x == 0) lost = 0u;
    const int64_t px0 = (int64_t)b * P, first = offs[b], end = min(offs[b + 1], total);
    uint8_t *out = payload + (int64_t)b * stride;
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
            if (p0 + k >= P) continue;
            uint32_t q = 0u;
            float w = 0.0f;
            if (set[k]) {
                const int32_t own = owner[px0 + p0 + k];
                const int64_t row = first + own;
                if (own == INT_NO_OWNER || row < 0 || row < first || row >= end) mylost++;   // ri is not the image of these rows
                else { w = rows[4 * row + 3]; q = intensity_quantise(w, scale); }
                out[8 + rank] = (uint8_t)q;   // rank < the frame's non-empty pixels <= P: inside the row of 8 + P bytes
                rank++;
            }
            if (image) image[px0 + p0 + k] = (uint8_t)q;
            if (owner_w) owner_w[px0 + p0 + k] = w;
        }
        running += all;
    }
    if (mylost) atomicAdd(&lost, mylost);
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t sb = f2u(scale);
        out[0] = 'R'; out[1] = 'P'; out[2] = 'I'; out[3] = '1';
        out[4] = (uint8_t)sb; out[5] = (uint8_t)(sb >> 8); out[6] = (uint8_t)(sb >> 16); out[7] = (uint8_t)(sb >> 24);
        nbytes[b] = 8 + (int32_t)running;
        orphans[b] = (int32_t)lost;
    }
}

template <class L>
__global__ __launch_bounds__(INT_FRAME_THREADS) void intensity_decode_kernel(const uint8_t *__restrict__ payload, int64_t stride, const int32_t *__restrict__ nbytes,
                                                                              const L *__restrict__ labels, int P, float *__restrict__ intensity,
                                                                              int32_t *__restrict__ status) {
    __shared__ uint32_t wsum[INT_FRAME_THREADS / 64];
    const int b = blockIdx.x;
    const int64_t px0 = (int64_t)b * P;
    const uint8_t *in = payload + (int64_t)b * stride;
    const int64_t nb = nbytes[b];
    // the header is read only when the row holds one
    bool ok = nb >= 8 && nb <= stride && nb - 8 <= P;
    float scale = 1.0f;
    if (ok) {
        const uint32_t magic = (uint32_t)in[0] | (uint32_t)in[1] << 8 | (uint32_t)in[2] << 16 | (uint32_t)in[3] << 24;
        scale = u2f((uint32_t)in[4] | (uint32_t)in[5] << 8 | (uint32_t)in[6] << 16 | (uint32_t)in[7] << 24);
        ok = magic == INT_MAGIC && scale > 0.0f && scale <= 3.402823466e+38f;
    }
    // the number of pixels with a label other than 1 is what the payload must hold
    uint32_t mine = 0u;
    for (int p = threadIdx.x; p < P; p += INT_FRAME_THREADS) mine += labels[px0 + p] != (L)1 ? 1u : 0u;
    uint32_t n;
    (void)intensity_block_scan(mine, wsum, n);
    ok = ok && (int64_t)n == nb - 8;   // (workgroup-uniform)
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
            float w = 0.0f;
            if (set[k]) { w = (float)in[8 + rank] / scale; rank++; }   // rank < n = nbytes - 8 <= stride - 8
            intensity[px0 + p0 + k] = w;
        }
        running += all;
    }
    if (threadIdx.x == 0) status[b] = ok ? RPCC_STREAM_OK : RPCC_STREAM_E_INTENSITY;
}
