// lz4_kernels.hip -- librpcc_lz4.so (include/rpcc_lz4.h): LZ4 block encode / decode and .rpcc container compaction for
// gfx950.  The encoder follows DESIGN.md section 11 bit for bit; tests/lz4_ref.py is its numpy statement.
//
// Encoder: one 256-thread workgroup per stream.  The shared match finder (csrc_lzmatch/lz_match.h) walks the stream in tiles of
// 1024 positions and leaves each tile's sequences in LDS; they are sized, scanned and written by the whole workgroup.
//
// Decoder: one wavefront per stream.  The token stream is read through a 2 KB LDS window; literals are copied by all lanes
// from global memory; the last 64 KB of output are kept in an LDS ring, from which matches are served, so no lane reads back
// through global memory what the wave has just stored.  Every read is checked against the stream's length and every write
// against the header's size, which is checked against the capacity first.
#include "../../include/rpcc_lz4.h"
#include "../csrc_lzmatch/lz_match.h"
#include "../csrc_tile/tiles.h"

static_assert(RPCC_LZ4_ERR_ARG == TILE_ERR_ARG && RPCC_LZ4_ERR_HIP == TILE_ERR_HIP, "rpcc_lz4.h and tiles.h disagree");

#define MAX_OFFSET 65535
#define DEC_WINDOW 2048              // bytes of the decoder's token window
#define RING 65536                   // the decoder's history ring (> MAX_OFFSET)

extern "C" int rpcc_lz4_version(void) { return RPCC_LZ4_ABI_VERSION; }
extern "C" const char *rpcc_lz4_last_error(void) { return g_err; }

__host__ __device__ static inline int64_t lz4_bound(int64_t n) { return 4 + n + n / 255 + 16; }

// ------------------------------------------------------------------------------------------------
// encoder
// ------------------------------------------------------------------------------------------------
// Bytes of a length's continuation: lengths >= 15 continue in 255-bytes and a final byte < 255.
__device__ __forceinline__ uint32_t ext_bytes(uint32_t v) { return v >= 15 ? (v - 15) / 255 + 1 : 0; }

__device__ __forceinline__ uint32_t put_ext(uint8_t *o, uint32_t v) {   // -> bytes written
    if (v < 15) return 0;
    uint32_t r = v - 15, k = 0;
    for (; r >= 255; r -= 255) o[k++] = 255;
    o[k++] = (uint8_t)r;
    return k;
}

struct EncShared {
    MatchShared m;
    uint32_t lit_out[ENC_SEQ];       // where each sequence's literals go
    uint32_t wsum[ENC_THREADS / 64];
};

__global__ __launch_bounds__(ENC_THREADS) void encode_kernel(const uint64_t *__restrict__ src_ptr, const int64_t *__restrict__ src_len,
                                                            uint8_t *__restrict__ dst, const int64_t *__restrict__ dst_off,
                                                            const int64_t *__restrict__ dst_cap, int64_t *__restrict__ dst_len) {
    __shared__ EncShared S;
    const int64_t s = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t n64 = src_len[s];
    if (n64 < 0 || n64 > RPCC_LZ4_MAX_INPUT || dst_cap[s] < lz4_bound(n64)) {
        if (tid == 0) dst_len[s] = RPCC_LZ4_E_CAPACITY;
        return;
    }
    const uint32_t n = (uint32_t)n64;
    const uint8_t *__restrict__ src = (const uint8_t *)src_ptr[s];
    uint8_t *__restrict__ out = dst + dst_off[s];
    if (tid < 4) out[tid] = (uint8_t)(n >> (8 * tid));
    uint32_t op = 4;                                    // output position in the slot
    const uint32_t m = match_positions(n);
    match_init(S.m);

    for (uint32_t t0 = 0; t0 < m; t0 += ENC_TILE) {
        match_tile<MAX_OFFSET>(S.m, src, n, t0, min((uint32_t)ENC_TILE, m - t0));
        const uint32_t nseq = S.m.nseq;
        if (nseq) {   // the tile's sequences: sizes, scan, headers by one thread each, literals by one wave each
            uint4 q = make_uint4(0, 0, 0, 0);
            uint32_t size = 0;
            if ((uint32_t)tid < nseq) {
                q = S.m.seq[tid];
                size = 1 + ext_bytes(q.y) + q.y + 2 + ext_bytes(q.w - 4);
            }
            uint32_t total;
            const uint32_t at = op + block_scan256(size, S.wsum, &total);
            if ((uint32_t)tid < nseq) {
                uint8_t *o = out + at;
                const uint32_t ml = q.w - 4;
                *o++ = (uint8_t)(min(q.y, 15u) << 4 | min(ml, 15u));
                o += put_ext(o, q.y);
                S.lit_out[tid] = (uint32_t)(o - out);
                o += q.y;
                *o++ = (uint8_t)q.z;
                *o++ = (uint8_t)(q.z >> 8);
                put_ext(o, ml);
            }
            __syncthreads();
            for (uint32_t e = wave; e < nseq; e += ENC_THREADS / 64) {
                const uint4 r = S.m.seq[e];
                uint8_t *o = out + S.lit_out[e];
                for (uint32_t x = lane; x < r.y; x += 64) o[x] = src[r.x + x];
            }
            op += total;
        }
        __syncthreads();   // bytes / keys / seq are rewritten by the next tile
    }
    // the last literals src[anchor .. n)
    const uint32_t anchor = S.m.anchor, ll = n - anchor;
    const uint32_t hdr = 1 + ext_bytes(ll);
    if (tid == 0) {
        out[op] = (uint8_t)(min(ll, 15u) << 4);
        put_ext(out + op + 1, ll);
        dst_len[s] = (int64_t)op + hdr + ll;
    }
    for (uint32_t x = tid; x < ll; x += ENC_THREADS) out[op + hdr + x] = src[anchor + x];
}

// ------------------------------------------------------------------------------------------------
// container compaction
// ------------------------------------------------------------------------------------------------
// One workgroup: coff[k] = the container offset of stream k (exclusive scan of 4 + dst_len), frame offsets and lengths.
// A frame with a failed stream, or whose end passes out_cap, gets frame_len -1 and coff[k] = -1 for its streams.
__global__ __launch_bounds__(1024) void pack_scan_kernel(const int64_t *__restrict__ dst_len, int64_t nframes, int per_frame, int64_t out_cap,
                                                         int64_t *__restrict__ coff, int64_t *__restrict__ frame_off,
                                                         int64_t *__restrict__ frame_len) {
    __shared__ int64_t part[1024];
    __shared__ int64_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int64_t f0 = 0; f0 < nframes; f0 += 1024) {
        const int64_t f = f0 + threadIdx.x;
        int64_t len = 0;
        bool ok = f < nframes;
        if (ok) {
            for (int a = 0; a < per_frame; ++a) {
                const int64_t l = dst_len[f * per_frame + a];
                ok = ok && l >= 0;
                len += 4 + (l >= 0 ? l : 0);
            }
        }
        part[threadIdx.x] = ok ? len : 0;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {   // inclusive Hillis-Steele scan
            const int64_t y = threadIdx.x >= (unsigned)o ? part[threadIdx.x - o] : 0;
            __syncthreads();
            part[threadIdx.x] += y;
            __syncthreads();
        }
        if (f < nframes) {
            const int64_t end = carry + part[threadIdx.x], start = end - (ok ? len : 0);
            ok = ok && end <= out_cap;
            frame_off[f] = start;
            frame_len[f] = ok ? len : -1;
            int64_t at = start;
            for (int a = 0; a < per_frame; ++a) {
                const int64_t k = f * per_frame + a;
                coff[k] = ok ? at : -1;
                at += 4 + (ok ? dst_len[k] : 0);
            }
        }
        __syncthreads();
        if (threadIdx.x == 1023) carry += part[1023];
        __syncthreads();
    }
}

// One workgroup per stream: [int32 length | bytes] at coff[k].
__global__ __launch_bounds__(256) void pack_copy_kernel(const uint8_t *__restrict__ slots, const int64_t *__restrict__ dst_off,
                                                        const int64_t *__restrict__ dst_len, const int64_t *__restrict__ coff,
                                                        uint8_t *__restrict__ out) {
    const int64_t k = blockIdx.x, at = coff[k];
    if (at < 0) return;
    const int64_t len = dst_len[k];
    const uint8_t *s = slots + dst_off[k];
    uint8_t *o = out + at;
    if (threadIdx.x < 4) o[threadIdx.x] = (uint8_t)((uint32_t)len >> (8 * threadIdx.x));
    for (int64_t x = threadIdx.x; x < len; x += blockDim.x) o[4 + x] = s[x];
}

// ------------------------------------------------------------------------------------------------
// decoder
// ------------------------------------------------------------------------------------------------
struct DecShared {
    uint8_t ring[RING];            // output position x at ring[x & (RING - 1)]
    uint8_t win[DEC_WINDOW];       // input bytes [wb, wb + DEC_WINDOW)
};

__global__ __launch_bounds__(64) void decode_kernel(const uint64_t *__restrict__ src_ptr, const int64_t *__restrict__ src_len,
                                                    uint8_t *__restrict__ dst, const int64_t *__restrict__ dst_off,
                                                    const int64_t *__restrict__ dst_cap, int64_t *__restrict__ dst_len,
                                                    int32_t *__restrict__ status) {
    __shared__ DecShared S;
    const int64_t s = blockIdx.x;
    const int lane = threadIdx.x;
    const uint8_t *__restrict__ in = (const uint8_t *)src_ptr[s];
    const int64_t iend = src_len[s];
    uint8_t *__restrict__ out = dst + dst_off[s];
    int64_t op = 0;
    int st = RPCC_LZ4_OK;
    int64_t wb = -DEC_WINDOW;      // window base: empty
    // one input byte at ip < iend, through the window (every lane asks for the same ip)
    auto get = [&](int64_t ip) -> uint32_t {
        if (ip >= wb + DEC_WINDOW) {
            __syncthreads();
            wb = ip;
            for (int64_t x = lane; x < DEC_WINDOW && wb + x < iend; x += 64) S.win[x] = in[wb + x];
            __syncthreads();
        }
        return S.win[ip - wb];
    };
    do {
        if (iend < 4) {
            st = RPCC_LZ4_E_TRUNCATED;
            break;
        }
        const int64_t n = (int64_t)(get(0) | get(1) << 8 | get(2) << 16 | get(3) << 24);
        if (n > dst_cap[s]) {
            st = RPCC_LZ4_E_CAPACITY;
            break;
        }
        int64_t ip = 4;
        if (n == 0 && iend == 4) break;
        for (;;) {
            if (ip >= iend) {
                st = RPCC_LZ4_E_TRUNCATED;
                break;
            }
            const uint32_t tok = get(ip++);
            int64_t ll = tok >> 4;
            if (ll == 15) {
                uint32_t b = 255;
                while (b == 255 && ip < iend) {
                    b = get(ip++);
                    ll += b;
                }
                if (b == 255) {   // the input ends inside the length
                    st = RPCC_LZ4_E_TRUNCATED;
                    break;
                }
            }
            if (ll > iend - ip) {
                st = RPCC_LZ4_E_TRUNCATED;
                break;
            }
            if (ll > n - op) {
                st = RPCC_LZ4_E_OVERRUN;
                break;
            }
            for (int64_t x = lane; x < ll; x += 64) {
                const uint8_t b = in[ip + x];
                out[op + x] = b;
                S.ring[(op + x) & (RING - 1)] = b;
            }
            __syncthreads();
            ip += ll;
            op += ll;
            if (ip == iend) break;   // the block ends after a literal run
            if (iend - ip < 2) {
                st = RPCC_LZ4_E_TRUNCATED;
                break;
            }
            const int64_t off = get(ip) | get(ip + 1) << 8;
            ip += 2;
            if (off == 0 || off > op) {
                st = RPCC_LZ4_E_OFFSET;
                break;
            }
            int64_t ml = tok & 15;
            if (ml == 15) {
                uint32_t b = 255;
                while (b == 255 && ip < iend) {
                    b = get(ip++);
                    ml += b;
                }
                if (b == 255) {
                    st = RPCC_LZ4_E_TRUNCATED;
                    break;
                }
            }
            ml += 4;
            if (ml > n - op) {
                st = RPCC_LZ4_E_OVERRUN;
                break;
            }
            // out[op + k] = out[op - off + k].  P: the smallest multiple of off >= 64.  k < P reads the history before op
            // (periodic in off); k >= P reads op + k - P, written by an earlier 64-byte step.  Both lie within the last 64 KB.
            const int64_t P = off >= 64 ? off : off * ((63 + off) / off);
            for (int64_t base = 0; base < ml; base += 64) {
                const int64_t k = base + lane;
                if (k < ml) {
                    const int64_t from = k < P ? op - off + (off > k ? k : (uint32_t)k % (uint32_t)off) : op + k - P;
                    const uint8_t b = S.ring[from & (RING - 1)];
                    out[op + k] = b;
                    S.ring[(op + k) & (RING - 1)] = b;
                }
                __syncthreads();
            }
            op += ml;
        }
        if (st == RPCC_LZ4_OK && op != n) st = RPCC_LZ4_E_SIZE;
    } while (0);
    if (lane == 0) {
        status[s] = st;
        dst_len[s] = op;
    }
}

// ------------------------------------------------------------------------------------------------
// C entries
// ------------------------------------------------------------------------------------------------
extern "C" size_t rpcc_lz4_bound(int64_t n) { return n < 0 || n > RPCC_LZ4_MAX_INPUT ? 0 : (size_t)lz4_bound(n); }

extern "C" size_t rpcc_lz4_workspace_bytes(int64_t nstreams) {
    return nstreams < 0 || nstreams > RPCC_LZ4_MAX_STREAMS ? 0 : (size_t)(nstreams + 1) * 8;
}

extern "C" int rpcc_lz4_encode(const uint64_t *src_ptr, const int64_t *src_len, int64_t nstreams, uint8_t *dst, const int64_t *dst_off,
                               const int64_t *dst_cap, int64_t *dst_len, void *stream) {
    ARG_TRY(nstreams >= 0 && nstreams <= RPCC_LZ4_MAX_STREAMS);
    ARG_TRY(src_ptr && src_len && dst && dst_off && dst_cap && dst_len);
    if (nstreams == 0) return 0;
    hipLaunchKernelGGL(encode_kernel, dim3((unsigned)nstreams), dim3(ENC_THREADS), 0, (hipStream_t)stream, src_ptr, src_len, dst, dst_off,
                       dst_cap, dst_len);
    LAUNCH_CHECK();
    return 0;
}

extern "C" int rpcc_lz4_pack_containers(const uint8_t *slots, const int64_t *dst_off, const int64_t *dst_len, int64_t nframes, int per_frame,
                                        uint8_t *out, int64_t out_cap, int64_t *frame_off, int64_t *frame_len, void *ws, void *stream) {
    ARG_TRY(nframes >= 0 && per_frame >= 1 && per_frame <= 64 && nframes <= RPCC_LZ4_MAX_STREAMS / per_frame);
    ARG_TRY(out_cap >= 0);
    ARG_TRY(slots && dst_off && dst_len && out && frame_off && frame_len && ws);
    if (nframes == 0) return 0;
    const hipStream_t st = (hipStream_t)stream;
    int64_t *coff = (int64_t *)ws;
    hipLaunchKernelGGL(pack_scan_kernel, dim3(1), dim3(1024), 0, st, dst_len, nframes, per_frame, out_cap, coff, frame_off, frame_len);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(pack_copy_kernel, dim3((unsigned)(nframes * per_frame)), dim3(256), 0, st, slots, dst_off, dst_len, coff, out);
    LAUNCH_CHECK();
    return 0;
}

extern "C" int rpcc_lz4_decode(const uint64_t *src_ptr, const int64_t *src_len, int64_t nstreams, uint8_t *dst, const int64_t *dst_off,
                               const int64_t *dst_cap, int64_t *dst_len, int32_t *status, void *stream) {
    ARG_TRY(nstreams >= 0 && nstreams <= RPCC_LZ4_MAX_STREAMS);
    ARG_TRY(src_ptr && src_len && dst && dst_off && dst_cap && dst_len && status);
    if (nstreams == 0) return 0;
    hipLaunchKernelGGL(decode_kernel, dim3((unsigned)nstreams), dim3(64), 0, (hipStream_t)stream, src_ptr, src_len, dst, dst_off, dst_cap,
                       dst_len, status);
    LAUNCH_CHECK();
    return 0;
}
