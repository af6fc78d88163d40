// rans_kernels.hip -- librpcc_rans.so (include/rpcc_rans.h): the chunk-parallel rANS back-end for gfx950.  The format's rules -- the
// normalisation, the parsing of header, tables and directory, the coding of a chunk by one wavefront -- are csrc_rans/rans_core.h, which
// the host tests build too; this file is what surrounds them on the device: the launches, the tables in LDS, histograms and assembly.
//
// Encoder, six launches: plan (one workgroup: which streams are taken, a scan of their chunk groups), histogram (one wave per chunk, LDS
// atomics, added into the stream's counts), normalisation (one wave per stream and plane), chunk encoder (one wave per chunk into a
// worst-case scratch slot), assembly (one workgroup per stream: coded or stored, header, tables, directory, the chunks' places) and copy
// (one wave per chunk: its payload, or its bytes of a stored stream, into place).  A workgroup of 256 threads takes a group of four
// consecutive chunks of one stream, so the tables in LDS are built once per four chunks; the grid is one workgroup per group the host
// can bound -- total_bytes / (4 chunk) + nstreams -- and a workgroup finds its stream by bisection of the scanned group counts.
//
// Decoder, three launches: validation (one wave per stream: rans_parse), then the chunks twice -- decoded without stores, the lowest
// status of a stream's chunks joining its status, then decoded again with stores for the streams that are still OK -- so a refused stream
// writes nothing.  The entry has rpcc_lz4_decode's signature and so no capacity the host knows: the grid is DEC_GROUPS workgroups by
// nstreams, a workgroup leaves at once when its stream has no group for it and strides on when the stream has more.
//
// Version 2 (the delta filter, csrc_rans/rans_filter.h) keeps every launch and the work buffer: the histogram and the chunk encoder read
// their input through the forward filter as they load it (a lane's element and the one before it: no filtered copy exists anywhere), the
// assembly writes the 'RB' header where such a stream is coded, and the decoder's storing pass has the wave that stored a chunk undo
// the filter over it in place (a scan per 256 bytes); the checking pass and the validation read both versions alike.
#include "../../include/rpcc_rans.h"
#include "../csrc_tile/tiles.h"

static_assert(RPCC_RANS_ERR_ARG == TILE_ERR_ARG && RPCC_RANS_ERR_HIP == TILE_ERR_HIP, "rpcc_rans.h and tiles.h disagree");

__device__ __forceinline__ uint64_t wave_sum64(uint64_t v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ uint32_t wave_max32(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o));
    return v;
}
// Inclusive sum over lanes 0 .. lane, all 64 lanes active.  DPP: four shifts within the rows of 16 (lanes shifted in from outside a row
// read 0), then lane 15 of rows 0 and 2 added to rows 1 and 3 (row_bcast:15, row mask 0xA) and lane 31 to rows 2 and 3 (row_bcast:31,
// row mask 0xC); a row that is masked out adds the `old` operand, 0.
__device__ __forceinline__ uint32_t wave_scan32(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, true);   // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, true);   // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, true);   // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, true);   // row_shr:8
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false);  // row_bcast:15
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false);  // row_bcast:31
    return v;
}

#define RANS_FN __device__ __forceinline__
#define RANS_NL 1
#define RANS_EACH(l) for (int l = lane, l##_once = 1; l##_once; l##_once = 0)
#define RANS_AT(a, l) a[0]
#define RANS_BALLOT(a) ((uint64_t)__ballot((a)[0] != 0))
#define RANS_SUM64(a) wave_sum64((a)[0])
#define RANS_MAX32(a) wave_max32((a)[0])
#define RANS_SCAN32(a) ((a)[0] = wave_scan32((a)[0]))
#define RANS_LAST32(a) ((uint32_t)__shfl((int)(a)[0], 63))
#define RANS_SYNC()                                         \
    do {                                                     \
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); \
        __builtin_amdgcn_wave_barrier();                     \
    } while (0)
#include "rans_core.h"

#define THREADS 256
#define GROUP 4                   // chunks per workgroup: one per wave
#define DEC_GROUPS 8              // workgroups per stream in the decoder's grid
#define SLOT_BYTES(clog) (2 * ((size_t)1 << (clog)) + 256)   // a chunk's scratch slot: one word per byte at most, 64 states

extern "C" int rpcc_rans_version(void) { return RPCC_RANS_ABI_VERSION; }
extern "C" const char *rpcc_rans_last_error(void) { return g_err; }

// Exclusive scan of v over the 256 threads; *total: the sum.  s_w: 4 words of LDS.
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t *s_w, uint32_t *total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t inc = v;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(inc, o);
        if (lane >= o) inc += y;
    }
    __syncthreads();              // s_w may still be read from an earlier scan
    if (lane == 63) s_w[w] = inc;
    __syncthreads();
    uint32_t off = 0;
    for (int k = 0; k < w; ++k) off += s_w[k];
    *total = s_w[0] + s_w[1] + s_w[2] + s_w[3];
    return off + inc - v;
}

// Bytes [0, n) from s to d by one wave: dwords of any alignment, then the tail.
__device__ __forceinline__ void wave_copy(uint8_t *__restrict__ d, const uint8_t *__restrict__ s, uint32_t n, int lane) {
    for (uint32_t x = 4 * lane; x + 4 <= n; x += 256) rans_st32(d + x, rans_ld32(s + x));
    const uint32_t x = (n & ~3u) + lane;
    if (x < n) d[x] = s[x];
}

// ------------------------------------------------------------------------------------------------
// encoder
// ------------------------------------------------------------------------------------------------
struct EncWs {                    // the work buffer's parts (device pointers into ws)
    uint32_t *gbase;              // [nstreams + 1] first group of every stream
    int32_t *mode;                // [nstreams] -1 refused, 0 stored, 1 coded
    uint32_t *pay;                // [nstreams] where a coded stream's payloads start
    uint32_t *counts;             // [nstreams][4][256]
    uint16_t *freq;               // [nstreams][4][256]
    uint32_t *clen, *coff;        // [gmax * GROUP] a chunk's payload length and its offset among its stream's payloads
    uint8_t *scratch;             // [gmax * GROUP] slots
    int64_t gmax;
    size_t bytes;
};

static EncWs enc_layout(void *ws, int64_t nstreams, int64_t total, int clog) {
    EncWs W;
    W.gmax = total / ((int64_t)GROUP << clog) + nstreams;
    size_t at = 0;
    uint8_t *b = (uint8_t *)ws;
    auto take = [&](size_t n) {
        uint8_t *p = b + at;
        at += al(n);
        return p;
    };
    W.gbase = (uint32_t *)take(4 * (size_t)(nstreams + 1));
    W.mode = (int32_t *)take(4 * (size_t)nstreams);
    W.pay = (uint32_t *)take(4 * (size_t)nstreams);
    W.counts = (uint32_t *)take(4096 * (size_t)nstreams);
    W.freq = (uint16_t *)take(2048 * (size_t)nstreams);
    W.clen = (uint32_t *)take(4 * (size_t)W.gmax * GROUP);
    W.coff = (uint32_t *)take(4 * (size_t)W.gmax * GROUP);
    W.scratch = take((size_t)W.gmax * GROUP * SLOT_BYTES(clog));
    W.bytes = at;
    return W;
}

// A stream's width word (rpcc_rans.h): bits 0-7 the element size, bits 8-15 the filter; plan_kernel takes only words whose other bits are 0.
__device__ __forceinline__ int32_t word_of(const int32_t *width, int64_t s) { return width ? width[s] : 1; }
__device__ __forceinline__ int32_t width_of(const int32_t *width, int64_t s) { return RPCC_RANS_WIDTH_OF(word_of(width, s)); }
__device__ __forceinline__ uint32_t filter_of(const int32_t *width, int64_t s) { return (uint32_t)RPCC_RANS_FILTER_OF(word_of(width, s)); }
__device__ __forceinline__ uint32_t chunks_of(uint32_t n, int clog) { return (uint32_t)(((uint64_t)n + (1u << clog) - 1) >> clog); }

// One workgroup: mode[s] = -1 and dst_len[s] = E_CAPACITY for a stream that is not taken; gbase = the exclusive scan of the taken streams'
// group counts, held at gmax (a stream whose groups end beyond gmax is not taken: the lengths add up to more than total_bytes).
__global__ __launch_bounds__(1024) void plan_kernel(const int64_t *__restrict__ src_len, const int32_t *__restrict__ width,
                                                    const int64_t *__restrict__ dst_cap, int64_t nstreams, int64_t gmax, int clog, EncWs W,
                                                    int64_t *__restrict__ dst_len) {
    __shared__ int64_t part[1024];
    __shared__ int64_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int64_t s0 = 0; s0 < nstreams; s0 += 1024) {
        const int64_t s = s0 + threadIdx.x;
        int64_t g = 0;
        bool ok = false;
        if (s < nstreams) {
            const int64_t n = src_len[s];
            const int32_t word = word_of(width, s), w = RPCC_RANS_WIDTH_OF(word), f = RPCC_RANS_FILTER_OF(word);
            ok = n >= 0 && n <= RPCC_RANS_MAX_INPUT && word == RPCC_RANS_WIDTH_WORD(w, f) && (w == 1 || w == 2 || w == 4) &&
                 (f == RPCC_RANS_FILTER_NONE || f == RPCC_RANS_FILTER_DELTA) && dst_cap[s] >= RANS_HEADER + n;
            if (ok) g = (chunks_of((uint32_t)n, clog) + GROUP - 1) / GROUP;
        }
        part[threadIdx.x] = g;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {   // inclusive Hillis-Steele scan
            const int64_t y = threadIdx.x >= (unsigned)o ? part[threadIdx.x - o] : 0;
            __syncthreads();
            part[threadIdx.x] += y;
            __syncthreads();
        }
        if (s < nstreams) {
            const int64_t end = carry + part[threadIdx.x];
            ok = ok && end <= gmax;
            W.gbase[s] = (uint32_t)min(end - g, gmax);
            W.mode[s] = ok ? 0 : -1;
            if (!ok) dst_len[s] = RPCC_RANS_E_CAPACITY;
        }
        __syncthreads();
        if (threadIdx.x == 1023) carry += part[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0) W.gbase[nstreams] = (uint32_t)min(carry, gmax);
}

// The stream of group g: the last s with gbase[s] <= g, or -1 when g is beyond the groups in use or the stream is not taken.
__device__ __forceinline__ int64_t stream_of(const EncWs &W, int64_t nstreams, uint32_t g) {
    if (g >= W.gbase[nstreams]) return -1;
    int64_t lo = 0, hi = nstreams - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (W.gbase[mid] <= g) lo = mid;
        else hi = mid - 1;
    }
    return W.mode[lo] < 0 ? -1 : lo;
}

__global__ __launch_bounds__(THREADS) void hist_kernel(const uint64_t *__restrict__ src_ptr, const int64_t *__restrict__ src_len,
                                                       const int32_t *__restrict__ width, int64_t nstreams, int clog, EncWs W) {
    __shared__ uint32_t h[4][256];
    const int64_t s = stream_of(W, nstreams, blockIdx.x);
    if (s < 0) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t n = (uint32_t)src_len[s], wd = (uint32_t)width_of(width, s);
    const uint32_t c = (blockIdx.x - W.gbase[s]) * GROUP + wave;
    for (int p = 0; p < 4; ++p) h[p][threadIdx.x] = 0;
    __syncthreads();
    if (c < chunks_of(n, clog)) {
        const uint8_t *__restrict__ src = (const uint8_t *)src_ptr[s] + ((size_t)c << clog);
        const uint32_t k = min(1u << clog, n - (c << clog));
        const bool delta = filter_of(width, s) == RANS_FILTER_DELTA;   // the bytes are counted as the coder will see them: through the filter
        for (uint32_t x = 4 * lane; x + 4 <= k; x += 256) {     // x is a multiple of 4: byte x + j is in plane j mod width
            uint32_t v = rans_ld32(src + x);
            if (delta) v = rans_delta_dword(v, x ? rans_ld_elem(src + x - wd, wd) : 0u, wd);
            for (uint32_t j = 0; j < 4; ++j) atomicAdd(&h[j & (wd - 1)][(v >> (8 * j)) & 255u], 1u);
        }
        const uint32_t x = (k & ~3u) + lane;
        if (x < k) atomicAdd(&h[x & (wd - 1)][delta ? rans_delta_byte(src, x, k, wd) : src[x]], 1u);
    }
    __syncthreads();
    for (uint32_t p = 0; p < wd; ++p)
        if (h[p][threadIdx.x]) atomicAdd(&W.counts[((size_t)s * 4 + p) * 256 + threadIdx.x], h[p][threadIdx.x]);
}

__global__ __launch_bounds__(64) void norm_kernel(const int64_t *__restrict__ src_len, const int32_t *__restrict__ width, EncWs W) {
    const int64_t s = blockIdx.x >> 2;
    const uint32_t p = blockIdx.x & 3;
    const int lane = threadIdx.x;
    if (W.mode[s] < 0 || p >= (uint32_t)width_of(width, s)) return;
    const uint32_t total = rans_plane_bytes((uint32_t)src_len[s], (uint32_t)width_of(width, s), p);
    uint16_t *freq = W.freq + ((size_t)s * 4 + p) * 256;
    if (total) rans_normalise(lane, W.counts + ((size_t)s * 4 + p) * 256, total, freq);
    else
        for (int j = 0; j < 4; ++j) freq[4 * lane + j] = 0;
}

__global__ __launch_bounds__(THREADS) void enc_kernel(const uint64_t *__restrict__ src_ptr, const int64_t *__restrict__ src_len,
                                                      const int32_t *__restrict__ width, int64_t nstreams, int clog, EncWs W) {
    __shared__ uint32_t enc[4 * 256 * 2];
    __shared__ uint32_t s_w[4];
    const int64_t s = stream_of(W, nstreams, blockIdx.x);
    if (s < 0) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t n = (uint32_t)src_len[s], wd = (uint32_t)width_of(width, s);
    for (uint32_t p = 0; p < wd; ++p) {
        const uint32_t f = W.freq[((size_t)s * 4 + p) * 256 + threadIdx.x];
        uint32_t total;
        const uint32_t cum = block_scan(f, s_w, &total);
        if (f) rans_enc_entry(f, cum, enc + (p * 256 + threadIdx.x) * 2);
    }
    __syncthreads();
    const uint32_t c = (blockIdx.x - W.gbase[s]) * GROUP + wave;
    if (c >= chunks_of(n, clog)) return;
    const size_t slot = (size_t)blockIdx.x * GROUP + wave;
    const uint32_t k = min(1u << clog, n - (c << clog));
    const uint32_t len = rans_encode_chunk_filtered(lane, (const uint8_t *)src_ptr[s] + ((size_t)c << clog), k, wd, filter_of(width, s), enc,
                                                    W.scratch + (slot + 1) * SLOT_BYTES(clog));
    if (lane == 0) W.clen[slot] = len;
}

// One workgroup per stream: the form (coded when smaller than 12 + n), header, tables and directory, the chunks' places.
__global__ __launch_bounds__(THREADS) void assemble_kernel(const int64_t *__restrict__ src_len, const int32_t *__restrict__ width, int clog, EncWs W,
                                                           uint8_t *__restrict__ dst, const int64_t *__restrict__ dst_off,
                                                           int64_t *__restrict__ dst_len) {
    __shared__ uint32_t s_w[4];
    __shared__ uint64_t s_sum;
    const int64_t s = blockIdx.x;
    if (W.mode[s] < 0) return;
    const uint32_t n = (uint32_t)src_len[s], wd = (uint32_t)width_of(width, s), nch = chunks_of(n, clog), tid = threadIdx.x;
    uint8_t *__restrict__ out = dst + dst_off[s];
    uint32_t f[4] = {0, 0, 0, 0}, rank[4], m[4] = {0, 0, 0, 0};
    uint64_t head = RANS_HEADER + 4 * (uint64_t)nch;
    for (uint32_t p = 0; p < wd; ++p) {
        f[p] = W.freq[((size_t)s * 4 + p) * 256 + tid];
        rank[p] = block_scan(f[p] != 0, s_w, &m[p]);
        head += 2 + 3 * m[p];
    }
    const size_t slot0 = (size_t)W.gbase[s] * GROUP;
    uint64_t paid = 0;                       // the payload bytes before this block of chunks
    for (uint32_t c0 = 0; c0 < nch; c0 += THREADS) {
        const uint32_t len = c0 + tid < nch ? W.clen[slot0 + c0 + tid] : 0;
        uint32_t total;
        const uint32_t off = block_scan(len, s_w, &total);     // (a block's lengths: 256 slots of at most 2^17 + 256 bytes)
        if (c0 + tid < nch) W.coff[slot0 + c0 + tid] = (uint32_t)(paid + off);   // meaningful where the stream is coded: paid < 2^31 then
        paid += total;
    }
    const bool coded = n > 0 && head + paid < RANS_HEADER + (uint64_t)n;
    if (tid == 0) {
        const uint32_t filter = filter_of(width, s);      // a filtered stream that does not shrink is the version-1 stored stream
        if (coded && filter != RANS_FILTER_NONE) rans_put_header_filtered(out, wd, n, clog, filter);
        else rans_put_header(out, coded, wd, n, clog);
        W.mode[s] = coded;
        W.pay[s] = (uint32_t)head;
        dst_len[s] = coded ? (int64_t)(head + paid) : RANS_HEADER + (int64_t)n;
    }
    if (!coded) return;
    uint32_t at = RANS_HEADER;
    for (uint32_t p = 0; p < wd; ++p) {
        if (tid == 0) rans_st16(out + at, m[p]);
        if (f[p]) {
            uint8_t *e = out + at + 2 + 3 * rank[p];
            e[0] = (uint8_t)tid;
            rans_st16(e + 1, f[p] - 1);
        }
        at += 2 + 3 * m[p];
    }
    for (uint32_t c = tid; c < nch; c += THREADS) rans_st32(out + at + 4 * (size_t)c, W.clen[slot0 + c]);
}

__global__ __launch_bounds__(THREADS) void copy_kernel(const uint64_t *__restrict__ src_ptr, const int64_t *__restrict__ src_len, int64_t nstreams,
                                                       int clog, EncWs W, uint8_t *__restrict__ dst, const int64_t *__restrict__ dst_off) {
    const int64_t s = stream_of(W, nstreams, blockIdx.x);
    if (s < 0) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t n = (uint32_t)src_len[s];
    const uint32_t c = (blockIdx.x - W.gbase[s]) * GROUP + wave;
    if (c >= chunks_of(n, clog)) return;
    const size_t slot = (size_t)blockIdx.x * GROUP + wave;
    uint8_t *__restrict__ out = dst + dst_off[s];
    if (W.mode[s] == 1) {
        const uint32_t len = W.clen[slot];
        wave_copy(out + W.pay[s] + W.coff[slot], W.scratch + (slot + 1) * SLOT_BYTES(clog) - len, len, lane);
    } else {
        const uint32_t k = min(1u << clog, n - (c << clog));
        wave_copy(out + RANS_HEADER + ((size_t)c << clog), (const uint8_t *)src_ptr[s] + ((size_t)c << clog), k, lane);
    }
}

// ------------------------------------------------------------------------------------------------
// decoder
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void validate_kernel(const uint64_t *__restrict__ src_ptr, const int64_t *__restrict__ src_len,
                                                      const int64_t *__restrict__ dst_cap, int64_t *__restrict__ dst_len,
                                                      int32_t *__restrict__ status) {
    const int64_t s = blockIdx.x;
    const int lane = threadIdx.x;
    RansInfo I;
    const int64_t len = src_len[s];
    const int st = len < 0 ? RPCC_RANS_E_TRUNCATED : rans_parse(lane, (const uint8_t *)src_ptr[s], len, dst_cap[s], I);
    if (lane == 0) {
        status[s] = st;
        dst_len[s] = st == RPCC_RANS_OK ? (int64_t)I.n : 0;
    }
}

struct DecShared {
    uint8_t lookup[4 * RANS_PROB];     // per plane: slot -> symbol
    uint32_t fc[4 * 256];              // per plane and symbol: rans_dec_entry
    uint32_t ring[GROUP][RANS_RING / 2];   // a wave's payload words, two to a dword
    uint16_t cum[257];                 // the table being built: entry -> cumulative frequency, 4096 behind the last
    uint8_t sym[256];
    uint32_t s_w[4];
};

// WRITE false: the chunks are decoded without stores and the lowest status joins status[s]; true: the streams still OK are written.
template <bool WRITE>
__global__ __launch_bounds__(THREADS) void dec_kernel(const uint64_t *__restrict__ src_ptr, uint8_t *__restrict__ dst,
                                                      const int64_t *__restrict__ dst_off, int64_t *__restrict__ dst_len,
                                                      int32_t *__restrict__ status) {
    __shared__ DecShared S;
    const int64_t s = blockIdx.y;
    const int32_t before = status[s];   // (the check's own E_STATE / E_PAYLOAD do not end it: the lowest of all chunks' statuses is wanted)
    if (WRITE ? before != RPCC_RANS_OK : before < 0 && before > RPCC_RANS_E_STATE) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, tid = threadIdx.x;
    const uint8_t *__restrict__ in = (const uint8_t *)src_ptr[s];
    RansInfo I;
    rans_read_header(in, RANS_HEADER, I);
    const uint32_t nch = chunks_of(I.n, (int)I.chunk_log2), size = 1u << I.chunk_log2;
    if (blockIdx.x * GROUP >= nch) return;
    uint8_t *__restrict__ out = dst + dst_off[s];
    if (I.mode == 0) {
        if (WRITE)
            for (uint32_t c = blockIdx.x * GROUP + wave; c < nch; c += DEC_GROUPS * GROUP)
                wave_copy(out + (size_t)c * size, in + RANS_HEADER + (size_t)c * size, min(size, I.n - c * size), lane);
        return;
    }
    rans_layout(in, I);
#pragma unroll
    for (uint32_t p = 0; p < 4; ++p) {
        if (p >= I.width) break;
        const uint32_t m = I.m[p];
        if (m == 0) continue;                  // (a plane without bytes: n < width)
        uint32_t f = 0, sy = 0;
        if ((uint32_t)tid < m) {
            const uint8_t *q = in + I.tab[p] + 3 * tid;
            sy = q[0], f = rans_ld16(q + 1) + 1;
        }
        uint32_t total;
        const uint32_t cum = block_scan(f, S.s_w, &total);
        __syncthreads();                       // the table of the plane before is read no more
        if ((uint32_t)tid < m) {
            S.fc[p * 256 + sy] = rans_dec_entry(f, cum);
            S.cum[tid] = (uint16_t)cum, S.sym[tid] = (uint8_t)sy;
        }
        if (tid == 0) S.cum[m] = RANS_PROB;
        __syncthreads();
        // 16 slots per thread: the entry of the first by bisection, then onwards (the frequencies sum to 4096: validated)
        uint32_t slot = 16 * tid, lo = 0, hi = m - 1;
        while (lo < hi) {
            const uint32_t mid = (lo + hi + 1) >> 1;
            if (S.cum[mid] <= slot) lo = mid;
            else hi = mid - 1;
        }
        for (uint32_t j = 0; j < 16; ++j, ++slot) {
            while (S.cum[lo + 1] <= slot) ++lo;
            S.lookup[p * RANS_PROB + slot] = S.sym[lo];
        }
    }
    __syncthreads();
    for (uint32_t c = blockIdx.x * GROUP + wave; c < nch; c += DEC_GROUPS * GROUP) {
        const int64_t at = rans_chunk_offset(lane, in, I, c);
        const uint32_t k = min(size, I.n - c * size);
        const int st = rans_decode_chunk(lane, in + at, rans_ld32(in + I.dir + 4 * (int64_t)c), k, I.width, S.lookup, S.fc, S.ring[wave],
                                         WRITE ? out + (size_t)c * size : nullptr);
        if (WRITE && I.filter == RANS_FILTER_DELTA) {   // version 2: the wave undoes the filter over the chunk it has just stored
            RANS_SYNC();
            rans_unfilter_chunk(lane, out + (size_t)c * size, k, I.width);
        }
        if (!WRITE && st != RPCC_RANS_OK && lane == 0) {
            atomicMin(&status[s], st);
            dst_len[s] = 0;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// C entries
// ------------------------------------------------------------------------------------------------
extern "C" size_t rpcc_rans_bound(int64_t n) { return n < 0 || n > RPCC_RANS_MAX_INPUT ? 0 : (size_t)(RANS_HEADER + n); }

static bool enc_args_ok(int64_t nstreams, int64_t total, int clog) {
    return nstreams >= 0 && nstreams <= RPCC_RANS_MAX_STREAMS && total >= 0 && total <= (int64_t)RPCC_RANS_MAX_INPUT * 64 &&
           clog >= RANS_MIN_CHUNK_LOG2 && clog <= RANS_MAX_CHUNK_LOG2 && total / ((int64_t)GROUP << clog) + nstreams <= 0x7FFFFFFF;
}

extern "C" size_t rpcc_rans_workspace_bytes(int64_t nstreams, int64_t total_bytes, int chunk_log2) {
    return enc_args_ok(nstreams, total_bytes, chunk_log2) ? enc_layout(nullptr, nstreams, total_bytes, chunk_log2).bytes : 0;
}

extern "C" int rpcc_rans_encode(const uint64_t *src_ptr, const int64_t *src_len, const int32_t *width, int64_t nstreams, int64_t total_bytes,
                                int chunk_log2, uint8_t *dst, const int64_t *dst_off, const int64_t *dst_cap, int64_t *dst_len, void *ws,
                                void *stream) {
    ARG_TRY(enc_args_ok(nstreams, total_bytes, chunk_log2));
    ARG_TRY(src_ptr && src_len && dst && dst_off && dst_cap && dst_len && ws);
    ARG_TRY(((uintptr_t)ws & 15) == 0);
    if (nstreams == 0) return 0;
    const hipStream_t st = (hipStream_t)stream;
    const EncWs W = enc_layout(ws, nstreams, total_bytes, chunk_log2);
    const dim3 groups((unsigned)W.gmax);
    HIP_TRY(hipMemsetAsync(W.counts, 0, 4096 * (size_t)nstreams, st));
    hipLaunchKernelGGL(plan_kernel, dim3(1), dim3(1024), 0, st, src_len, width, dst_cap, nstreams, W.gmax, chunk_log2, W, dst_len);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(hist_kernel, groups, dim3(THREADS), 0, st, src_ptr, src_len, width, nstreams, chunk_log2, W);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(norm_kernel, dim3((unsigned)(4 * nstreams)), dim3(64), 0, st, src_len, width, W);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(enc_kernel, groups, dim3(THREADS), 0, st, src_ptr, src_len, width, nstreams, chunk_log2, W);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(assemble_kernel, dim3((unsigned)nstreams), dim3(THREADS), 0, st, src_len, width, chunk_log2, W, dst, dst_off, dst_len);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(copy_kernel, groups, dim3(THREADS), 0, st, src_ptr, src_len, nstreams, chunk_log2, W, dst, dst_off);
    LAUNCH_CHECK();
    return 0;
}

extern "C" int rpcc_rans_decode(const uint64_t *src_ptr, const int64_t *src_len, int64_t nstreams, uint8_t *dst, const int64_t *dst_off,
                                const int64_t *dst_cap, int64_t *dst_len, int32_t *status, void *stream) {
    ARG_TRY(nstreams >= 0 && nstreams <= RPCC_RANS_MAX_STREAMS);
    ARG_TRY(src_ptr && src_len && dst && dst_off && dst_cap && dst_len && status);
    if (nstreams == 0) return 0;
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(validate_kernel, dim3((unsigned)nstreams), dim3(64), 0, st, src_ptr, src_len, dst_cap, dst_len, status);
    LAUNCH_CHECK();
    // the stream index is the grid's y: 65535 at most per launch
    for (int64_t s0 = 0; s0 < nstreams; s0 += 65535) {
        const dim3 grid(DEC_GROUPS, (unsigned)min((int64_t)65535, nstreams - s0));
        hipLaunchKernelGGL(dec_kernel<false>, grid, dim3(THREADS), 0, st, src_ptr + s0, dst, dst_off + s0, dst_len + s0, status + s0);
        LAUNCH_CHECK();
        hipLaunchKernelGGL(dec_kernel<true>, grid, dim3(THREADS), 0, st, src_ptr + s0, dst, dst_off + s0, dst_len + s0, status + s0);
        LAUNCH_CHECK();
    }
    return 0;
}
