// deflate_kernels.hip -- librpcc_deflate.so (include/rpcc_deflate.h): gzip members for gfx950.  The encoder follows DESIGN.md
// section 12 bit for bit; tests/deflate_ref.py is its numpy statement.
//
// Four launches per call, kernel boundaries being the fence between them:
//   prep    one workgroup: which streams are coded (length in range, slot >= bound) and where each one's records lie in the
//           workspace (an exclusive scan of n + 1 over the coded streams).
//   parse   one 256-thread workgroup per stream: the shared match finder (csrc_lzmatch/lz_match.h, window 32768) gives each
//           tile's sequences; every literal and every chunk of a match (<= 258 bytes) becomes one 32-bit record, placed by a
//           block scan of the sequences' record counts; 286 + 30 LDS counters take the symbols' frequencies; the CRC-32 of the
//           stream is folded 1 KB at a time (4 bytes per lane, combined by multiplication by x^(8k) mod the polynomial).
//   tables  one wavefront per stream: the three length-limited Huffman codes, the run-length coded header, the exact bit
//           total and the choice between the dynamic block and stored blocks.  The block header is written here.
//   emit    one 256-thread workgroup per stream: 1024 records at a time look up their <= 48 bits, a block scan of the bit
//           counts places them, they are ORed into a zeroed LDS stage and whole bytes leave together; the partial byte is
//           carried into the next 1024.  Stored blocks are a plain copy.
#include "../../include/rpcc_deflate.h"
#include "../csrc_lzmatch/lz_match.h"
#include "../csrc_tile/tiles.h"

static_assert(RPCC_DEFLATE_ERR_ARG == TILE_ERR_ARG && RPCC_DEFLATE_ERR_HIP == TILE_ERR_HIP, "rpcc_deflate.h and tiles.h disagree");

#define MAX_OFFSET 32768
#define MAX_MATCH 258
#define MIN_MATCH 3
#define NLIT 286                     // literal / length symbols
#define NDIST 30                     // distance symbols
#define NCL 19                       // code-length symbols
#define EOB 256
#define STORED_MAX 65535             // bytes of one stored block
#define GZ_HEADER 10
#define CRC_POLY 0xEDB88320u
#define CRC_CHUNK 1024               // bytes folded into the CRC per step
#define EMIT_ITEMS 4                 // records per thread and step of the emit kernel
#define EMIT_CHUNK (ENC_THREADS * EMIT_ITEMS)
#define REC_MATCH 0x80000000u        // record: a literal byte (or EOB), or REC_MATCH | (length - 3) << 16 | (distance - 1)
#define MAX_TOTAL ((int64_t)1 << 40) // total_len of one call

enum { KIND_NONE = 0, KIND_DYNAMIC = 1, KIND_STORED = 2 };

extern "C" int rpcc_deflate_version(void) { return RPCC_DEFLATE_ABI_VERSION; }
extern "C" const char *rpcc_deflate_last_error(void) { return g_err; }

__host__ __device__ static inline int64_t stored_blocks(int64_t n) { return n > STORED_MAX ? (n + STORED_MAX - 1) / STORED_MAX : 1; }
__host__ __device__ static inline int64_t deflate_bound(int64_t n) { return 18 + n + 5 * stored_blocks(n); }

// What the launches hand each other, one per stream.
struct StreamMeta {
    int64_t rec_off;                 // the stream's first record in the record area; -1: the stream is not coded
    uint64_t extra_bits;             // sum of the matches' extra bits
    uint32_t nrec;                   // records, the end-of-block record included (<= n + 1)
    uint32_t crc;
    uint32_t kind;                   // KIND_*
    uint32_t hdr_bits;               // bits of the dynamic block's header: the first record's code starts there
    uint32_t carry;                  // the header's last, partial byte
    uint32_t pad;
    uint32_t freq[NLIT + NDIST];
    uint32_t code[NLIT + NDIST];     // bit-reversed code | length << 16
};

// The workspace: what rpcc_deflate_workspace_bytes sizes and rpcc_deflate_encode carves.
struct WsLayout {
    size_t meta, recs, rec_words, bytes;
};
static WsLayout ws_layout(int64_t nstreams, int64_t total_len) {
    WsLayout L;
    L.meta = 0;
    L.recs = al((size_t)nstreams * sizeof(StreamMeta));
    L.rec_words = (size_t)total_len + (size_t)nstreams;   // n + 1 records per stream
    L.bytes = L.recs + L.rec_words * 4;
    return L;
}

// ------------------------------------------------------------------------------------------------
// symbols
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void length_symbol(uint32_t len, uint32_t &sym, uint32_t &eb, uint32_t &ev) {
    const uint32_t l = len - MIN_MATCH;
    if (l == 255) {
        sym = 285, eb = 0, ev = 0;
    } else if (l < 8) {
        sym = 257 + l, eb = 0, ev = 0;
    } else {
        const uint32_t hb = 31 - __clz(l);
        eb = hb - 2;
        sym = 257 + 4 * (hb - 1) + ((l >> eb) & 3);
        ev = l & ((1u << eb) - 1);
    }
}

__device__ __forceinline__ void distance_symbol(uint32_t dist, uint32_t &sym, uint32_t &eb, uint32_t &ev) {
    const uint32_t x = dist - 1;
    if (x < 4) {
        sym = x, eb = 0, ev = 0;
    } else {
        const uint32_t hb = 31 - __clz(x);
        eb = hb - 1;
        sym = 2 * hb + ((x >> eb) & 1);
        ev = x & ((1u << eb) - 1);
    }
}

// A match of length L leaves in chunks(L) deflate matches: 258s, and the last two so that neither is shorter than 3.
__device__ __forceinline__ uint32_t chunks(uint32_t L) { return (L + MAX_MATCH - 1) / MAX_MATCH; }
__device__ __forceinline__ uint32_t chunk_len(uint32_t L, uint32_t K, uint32_t j) {
    if (K == 1) return L;
    if (j + 2 < K) return MAX_MATCH;
    const uint32_t R = L - MAX_MATCH * (K - 2);   // 259 .. 516 for the last two
    if (R - MAX_MATCH >= MIN_MATCH) return j + 2 == K ? MAX_MATCH : R - MAX_MATCH;
    return j + 2 == K ? R - MIN_MATCH : MIN_MATCH;
}

// ------------------------------------------------------------------------------------------------
// CRC-32 (reflected: x^0 is bit 31)
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t gf_mul(uint32_t a, uint32_t b) {   // a * b mod the polynomial
    uint32_t p = 0;
    for (int i = 0; i < 32; ++i) {
        p ^= (a & (0x80000000u >> i)) ? b : 0;
        b = (b >> 1) ^ ((b & 1) ? CRC_POLY : 0);
    }
    return p;
}

// ------------------------------------------------------------------------------------------------
// prep
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void prep_kernel(const int64_t *__restrict__ src_len, const int64_t *__restrict__ dst_cap, int64_t nstreams,
                                                    int64_t rec_words, StreamMeta *__restrict__ meta, int64_t *__restrict__ dst_len) {
    __shared__ int64_t part[1024];
    __shared__ int64_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int64_t s0 = 0; s0 < nstreams; s0 += 1024) {
        const int64_t s = s0 + threadIdx.x;
        int64_t need = 0;
        if (s < nstreams) {
            const int64_t n = src_len[s];
            if (n >= 0 && n <= RPCC_DEFLATE_MAX_INPUT && dst_cap[s] >= deflate_bound(n)) need = n + 1;
        }
        part[threadIdx.x] = need;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {   // inclusive Hillis-Steele scan
            const int64_t y = threadIdx.x >= (unsigned)o ? part[threadIdx.x - o] : 0;
            __syncthreads();
            part[threadIdx.x] += y;
            __syncthreads();
        }
        if (s < nstreams) {
            const int64_t end = carry + part[threadIdx.x];
            const bool ok = need > 0 && end <= rec_words;
            meta[s].rec_off = ok ? end - need : -1;
            meta[s].kind = KIND_NONE;
            if (!ok) dst_len[s] = RPCC_DEFLATE_E_CAPACITY;
        }
        __syncthreads();
        if (threadIdx.x == 1023) carry += part[1023];
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------
// parse
// ------------------------------------------------------------------------------------------------
struct ParseShared {          // 79.4 KB: two workgroups per CU, as the LZ4 encoder
    MatchShared m;
    uint32_t rec_out[ENC_SEQ];       // where each sequence's records go
    uint32_t freq[NLIT + NDIST];
    uint32_t wsum[ENC_THREADS / 64];
    uint32_t wred[ENC_THREADS / 64];
    unsigned long long extra;
};

__device__ __forceinline__ uint32_t match_record(ParseShared &S, uint32_t len, uint32_t dist) {   // counts it, -> its extra bits
    uint32_t ls, le, lv, ds, de, dv;
    length_symbol(len, ls, le, lv);
    distance_symbol(dist, ds, de, dv);
    atomicAdd(&S.freq[ls], 1u);
    atomicAdd(&S.freq[NLIT + ds], 1u);
    return le + de;
}

__global__ __launch_bounds__(ENC_THREADS) void parse_kernel(const uint64_t *__restrict__ src_ptr, const int64_t *__restrict__ src_len,
                                                           StreamMeta *__restrict__ meta, uint32_t *__restrict__ recs) {
    __shared__ ParseShared S;
    const int64_t s = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t ro = meta[s].rec_off;
    if (ro < 0) return;
    const uint32_t n = (uint32_t)src_len[s];
    const uint8_t *__restrict__ src = (const uint8_t *)src_ptr[s];
    uint32_t *__restrict__ rec = recs + ro;
    for (int k = tid; k < NLIT + NDIST; k += ENC_THREADS) S.freq[k] = 0;
    if (tid == 0) S.extra = 0;
    // The CRC comes before the first tile, so its tables lie in the match finder's keys and cand: the byte table, and the powers
    // x^(8 j), j < 1024 (x^(32 tid) by squaring, then three steps of x^8); every thread keeps x^(8 * 1024).
    uint32_t *crc_tab = S.m.keys, *pw8 = S.m.cand;
    static_assert(CRC_CHUNK == ENC_TILE, "the CRC's tables take the place of one tile's keys and candidates");
    uint32_t pw_chunk;
    {
        uint32_t c = tid;
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1) ? CRC_POLY : 0);
        crc_tab[tid] = c;
        uint32_t r = 0x80000000u, b = CRC_POLY;   // x^0, x^32
        for (int k = 0; k < 8; ++k) {
            if ((tid >> k) & 1) r = gf_mul(r, b);
            b = gf_mul(b, b);
        }
        for (int k = 0; k < 4; ++k) {
            pw8[4 * tid + k] = r;
            r = gf_mul(r, 0x00800000u);   // x^8
        }
        pw_chunk = b;   // (x^32)^256
    }
    match_init(S.m);

    // CRC-32: the register after bytes B from state c is c * x^(8 |B|) + the register of B from state 0
    uint32_t crc = 0xFFFFFFFFu;
    for (uint32_t c0 = 0; c0 < n; c0 += CRC_CHUNK) {
        const uint32_t C = min((uint32_t)CRC_CHUNK, n - c0);
        const uint32_t lo = min(4u * tid, C), hi = min(4u * tid + 4, C);
        uint32_t r = 0;
        for (uint32_t x = lo; x < hi; ++x) r = crc_tab[(r ^ src[c0 + x]) & 255] ^ (r >> 8);
        r = gf_mul(r, pw8[C - hi]);
        for (int o = 32; o > 0; o >>= 1) r ^= __shfl_xor(r, o);
        if (lane == 0) S.wred[wave] = r;
        __syncthreads();
        crc = gf_mul(crc, C == CRC_CHUNK ? pw_chunk : pw8[C]) ^ S.wred[0] ^ S.wred[1] ^ S.wred[2] ^ S.wred[3];
        __syncthreads();
    }
    crc ^= 0xFFFFFFFFu;

    const uint32_t m = match_positions(n);
    uint32_t nrec = 0;
    uint64_t xb = 0;
    for (uint32_t t0 = 0; t0 < m; t0 += ENC_TILE) {
        match_tile<MAX_OFFSET>(S.m, src, n, t0, min((uint32_t)ENC_TILE, m - t0));
        const uint32_t nseq = S.m.nseq;
        if (nseq) {   // the tile's sequences: record counts, scan, then one wave per sequence writes and counts its records
            uint32_t cnt = 0;
            if ((uint32_t)tid < nseq) {
                const uint4 q = S.m.seq[tid];
                cnt = q.y + chunks(q.w);
            }
            uint32_t total;
            const uint32_t at = nrec + block_scan256(cnt, S.wsum, &total);
            if ((uint32_t)tid < nseq) S.rec_out[tid] = at;
            __syncthreads();
            for (uint32_t e = wave; e < nseq; e += ENC_THREADS / 64) {
                const uint4 r = S.m.seq[e];
                uint32_t *o = rec + S.rec_out[e];
                for (uint32_t x = lane; x < r.y; x += 64) {
                    const uint32_t b = src[r.x + x];
                    o[x] = b;
                    atomicAdd(&S.freq[b], 1u);
                }
                const uint32_t K = chunks(r.w);
                for (uint32_t j = lane; j < K; j += 64) {
                    const uint32_t len = chunk_len(r.w, K, j);
                    o[r.y + j] = REC_MATCH | (len - MIN_MATCH) << 16 | (r.z - 1);
                    xb += match_record(S, len, r.z);
                }
            }
            nrec += total;
        }
        __syncthreads();   // bytes / keys / seq are rewritten by the next tile
    }
    // the last literals src[anchor .. n), then end-of-block
    const uint32_t anchor = S.m.anchor, ll = n - anchor;
    for (uint32_t x = tid; x < ll; x += ENC_THREADS) {
        const uint32_t b = src[anchor + x];
        rec[nrec + x] = b;
        atomicAdd(&S.freq[b], 1u);
    }
    atomicAdd(&S.extra, (unsigned long long)xb);
    if (tid == 0) {
        rec[nrec + ll] = EOB;
        S.freq[EOB] = 1;
    }
    __syncthreads();
    for (int k = tid; k < NLIT + NDIST; k += ENC_THREADS) meta[s].freq[k] = S.freq[k];
    if (tid == 0) {
        meta[s].nrec = nrec + ll + 1;
        meta[s].crc = crc;
        meta[s].extra_bits = S.extra;
    }
}

// ------------------------------------------------------------------------------------------------
// tables
// ------------------------------------------------------------------------------------------------
#define MAX_LEAVES NLIT
struct TabShared {
    uint32_t f[NLIT + NDIST];                // frequencies (fewer than two used symbols are filled up)
    uint32_t fc[NCL];
    uint32_t weight[2 * MAX_LEAVES];         // leaves in sorted order, then internal nodes in creation order
    uint16_t parent[2 * MAX_LEAVES];
    uint16_t depth[2 * MAX_LEAVES];
    uint16_t order[MAX_LEAVES];              // the used symbols ascending by (f, symbol)
    uint32_t code[NLIT + NDIST];             // bit-reversed code | length << 16
    uint32_t ccode[NCL];
    uint16_t rl[NLIT + NDIST];               // code-length symbol | extra value << 5
    uint32_t num[16], next[16];
    uint8_t len[NLIT + NDIST];
    uint8_t clen[NCL];
    int nused;
};

// The code of an alphabet of nsym symbols with frequencies f (LDS): lengths to len, bit-reversed code | length << 16 to code.
// One wavefront; begins and ends with a barrier.
__device__ void huffman_code(TabShared &T, uint32_t *f, int nsym, int maxbits, uint8_t *len, uint32_t *code) {
    const int lane = threadIdx.x;
    __syncthreads();
    if (lane == 0) {
        int used = 0;
        for (int s = 0; s < nsym; ++s) used += f[s] > 0;
        for (int s = 0; used < 2; ++s)
            if (f[s] == 0) {
                f[s] = 1;
                ++used;
            }
        T.nused = used;
    }
    __syncthreads();
    for (int s = lane; s < nsym; s += 64) {   // rank sort by (f, symbol)
        len[s] = 0;
        code[s] = 0;
        const uint32_t fs = f[s];
        if (fs) {
            int r = 0;
            for (int t = 0; t < nsym; ++t) {
                const uint32_t ft = f[t];
                r += ft && (ft < fs || (ft == fs && t < s));
            }
            T.order[r] = (uint16_t)s;
            T.weight[r] = fs;
        }
    }
    __syncthreads();
    if (lane == 0) {
        const int n = T.nused;
        // two queues: on a tie between their heads the leaf goes first
        int li = 0, ii = n;
        for (int nw = n; nw < 2 * n - 1; ++nw) {
            uint32_t w = 0;
            for (int k = 0; k < 2; ++k) {
                int pick;
                if (li < n && (ii >= nw || T.weight[li] <= T.weight[ii])) pick = li++;
                else pick = ii++;
                w += T.weight[pick];
                T.parent[pick] = (uint16_t)nw;
            }
            T.weight[nw] = w;
        }
        T.depth[2 * n - 2] = 0;
        for (int k = 2 * n - 3; k >= 0; --k) T.depth[k] = T.depth[T.parent[k]] + 1;
        for (int i = 0; i <= maxbits; ++i) T.num[i] = 0;
        for (int k = 0; k < n; ++k) T.num[min((int)T.depth[k], maxbits)] += 1;
        uint32_t total = 0;
        for (int i = 1; i <= maxbits; ++i) total += T.num[i] << (maxbits - i);
        while (total != 1u << maxbits) {   // one leaf from the deepest level above maxbits that has one moves down, with a leaf from maxbits
            T.num[maxbits] -= 1;
            int i = maxbits - 1;
            while (T.num[i] == 0) --i;
            T.num[i] -= 1;
            T.num[i + 1] += 2;
            total -= 1;
        }
        int k = n;
        for (int i = 1; i <= maxbits; ++i)
            for (uint32_t c = 0; c < T.num[i]; ++c) len[T.order[--k]] = (uint8_t)i;
        uint32_t c = 0;
        T.num[0] = 0;
        for (int b = 1; b <= maxbits; ++b) {
            c = (c + T.num[b - 1]) << 1;
            T.next[b] = c;
        }
        for (int s = 0; s < nsym; ++s) {
            const uint32_t l = len[s];
            if (l) code[s] = (__brev(T.next[l]++) >> (32 - l)) | l << 16;
        }
    }
    __syncthreads();
}

__constant__ uint8_t CL_ORDER[NCL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

struct BitWriter {   // one lane, LSB first, whole bytes to memory
    uint8_t *o;
    uint64_t acc;
    uint32_t nbits, total;
    __device__ void put(uint32_t v, uint32_t b) {
        acc |= (uint64_t)v << nbits;
        nbits += b;
        total += b;
        while (nbits >= 8) {
            *o++ = (uint8_t)acc;
            acc >>= 8;
            nbits -= 8;
        }
    }
};

__global__ __launch_bounds__(64) void tables_kernel(const int64_t *__restrict__ src_len, uint8_t *__restrict__ dst,
                                                    const int64_t *__restrict__ dst_off, StreamMeta *__restrict__ meta) {
    __shared__ TabShared T;
    const int64_t s = blockIdx.x;
    const int lane = threadIdx.x;
    StreamMeta &M = meta[s];
    if (M.rec_off < 0) return;
    const int64_t n = src_len[s];
    uint8_t *__restrict__ out = dst + dst_off[s];
    for (int k = lane; k < NLIT + NDIST; k += 64) T.f[k] = M.freq[k];
    for (int k = lane; k < NCL; k += 64) T.fc[k] = 0;
    huffman_code(T, T.f, NLIT, 15, T.len, T.code);
    huffman_code(T, T.f + NLIT, NDIST, 15, T.len + NLIT, T.code + NLIT);
    __shared__ int s_hlit, s_hdist, s_nrl;
    if (lane == 0) {
        int hlit = NLIT, hdist = NDIST;
        while (hlit > 257 && T.len[hlit - 1] == 0) --hlit;
        while (T.len[NLIT + hdist - 1] == 0) --hdist;   // at least two distance codes have a length
        // the lengths of both alphabets as one sequence, run-length coded greedily from the left
        const int N = hlit + hdist;
        auto at = [&](int i) -> uint32_t { return i < hlit ? T.len[i] : T.len[NLIT + i - hlit]; };
        int nrl = 0;
        auto emit = [&](uint32_t sym, uint32_t ev) {
            T.rl[nrl++] = (uint16_t)(sym | ev << 5);
            T.fc[sym] += 1;
        };
        for (int i = 0; i < N;) {
            const uint32_t v = at(i);
            int r = 1;
            while (i + r < N && at(i + r) == v) ++r;
            if (v == 0) {
                if (r >= 11) {
                    const int t = min(r, 138);
                    emit(18, t - 11);
                    i += t;
                } else if (r >= 3) {
                    emit(17, r - 3);
                    i += r;
                } else {
                    emit(0, 0);
                    i += 1;
                }
            } else {
                emit(v, 0);
                int rest = r - 1;
                while (rest >= 3) {
                    const int t = min(rest, 6);
                    emit(16, t - 3);
                    rest -= t;
                }
                for (; rest > 0; --rest) emit(v, 0);
                i += r;
            }
        }
        s_hlit = hlit, s_hdist = hdist, s_nrl = nrl;
    }
    huffman_code(T, T.fc, NCL, 7, T.clen, T.ccode);
    for (int k = lane; k < NLIT + NDIST; k += 64) M.code[k] = T.code[k];
    if (lane < GZ_HEADER) out[lane] = lane == 0 ? 0x1F : lane == 1 ? 0x8B : lane == 2 ? 8 : lane == 9 ? 0xFF : 0;
    if (lane == 0) {
        const int hlit = s_hlit, hdist = s_hdist, nrl = s_nrl;
        int hclen = NCL;
        while (hclen > 4 && T.clen[CL_ORDER[hclen - 1]] == 0) --hclen;
        uint64_t bits = 3 + 14 + 3 * hclen;
        for (int k = 0; k < nrl; ++k) {
            const uint32_t sym = T.rl[k] & 31;
            bits += T.clen[sym] + (sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0);
        }
        const uint32_t hdr_bits = (uint32_t)bits;
        for (int k = 0; k < NLIT + NDIST; ++k) bits += (uint64_t)M.freq[k] * T.len[k];   // the counted symbols, not the filled-up ones
        bits += M.extra_bits;
        if ((bits + 7) / 8 <= (uint64_t)(n + 5 * stored_blocks(n))) {
            BitWriter w = {out + GZ_HEADER, 0, 0, 0};
            w.put(1, 1);
            w.put(2, 2);
            w.put(hlit - 257, 5);
            w.put(hdist - 1, 5);
            w.put(hclen - 4, 4);
            for (int k = 0; k < hclen; ++k) w.put(T.clen[CL_ORDER[k]], 3);
            for (int k = 0; k < nrl; ++k) {
                const uint32_t sym = T.rl[k] & 31;
                w.put(T.ccode[sym] & 0xFFFF, T.clen[sym]);
                w.put(T.rl[k] >> 5, sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0);
            }
            M.kind = KIND_DYNAMIC;
            M.hdr_bits = hdr_bits;   // == w.total
            M.carry = (uint32_t)w.acc;
        } else {
            M.kind = KIND_STORED;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// emit
// ------------------------------------------------------------------------------------------------
#define STAGE_WORDS (EMIT_CHUNK * 48 / 32 + 4)
struct EmitShared {
    uint32_t code[NLIT + NDIST];
    uint32_t stage[STAGE_WORDS];     // the chunk's bits, from the carried partial byte on
    uint32_t wsum[ENC_THREADS / 64];
};

__global__ __launch_bounds__(ENC_THREADS) void emit_kernel(const uint64_t *__restrict__ src_ptr, const int64_t *__restrict__ src_len,
                                                          uint8_t *__restrict__ dst, const int64_t *__restrict__ dst_off,
                                                          int64_t *__restrict__ dst_len, const StreamMeta *__restrict__ meta,
                                                          const uint32_t *__restrict__ recs) {
    __shared__ EmitShared S;
    const int64_t s = blockIdx.x;
    const int tid = threadIdx.x;
    const StreamMeta &M = meta[s];
    const uint32_t kind = M.kind;
    if (kind == KIND_NONE) return;
    const uint32_t n = (uint32_t)src_len[s];
    uint8_t *__restrict__ out = dst + dst_off[s];
    uint32_t opos;
    if (kind == KIND_STORED) {
        const uint8_t *__restrict__ src = (const uint8_t *)src_ptr[s];
        const uint32_t nb = (uint32_t)stored_blocks(n);
        for (uint32_t k = tid; k < nb; k += ENC_THREADS) {
            uint8_t *h = out + GZ_HEADER + (size_t)k * (STORED_MAX + 5);
            const uint32_t len = min((uint32_t)STORED_MAX, n - k * STORED_MAX);
            h[0] = k + 1 == nb ? 1 : 0;
            h[1] = (uint8_t)len, h[2] = (uint8_t)(len >> 8);
            h[3] = (uint8_t)~len, h[4] = (uint8_t)(~len >> 8);
        }
        for (uint32_t x = tid; x < n; x += ENC_THREADS) out[GZ_HEADER + 5 * (x / STORED_MAX + 1) + x] = src[x];
        opos = GZ_HEADER + n + 5 * nb;
    } else {
        for (int k = tid; k < NLIT + NDIST; k += ENC_THREADS) S.code[k] = M.code[k];
        const uint32_t *__restrict__ rec = recs + M.rec_off;
        const uint32_t nrec = M.nrec;
        uint32_t cb = M.hdr_bits & 7, carry = M.carry;   // bits and value of the partial byte at out[opos]
        opos = GZ_HEADER + (M.hdr_bits >> 3);
        for (uint32_t base = 0; base < nrec; base += EMIT_CHUNK) {
            for (int k = tid; k < STAGE_WORDS; k += ENC_THREADS) S.stage[k] = 0;
            if (tid == 0) S.stage[0] = carry;
            __syncthreads();   // and the code table, the first time
            uint64_t v[EMIT_ITEMS];
            uint32_t nb[EMIT_ITEMS], sum = 0;
#pragma unroll
            for (int j = 0; j < EMIT_ITEMS; ++j) {
                const uint32_t i = base + EMIT_ITEMS * tid + j;
                v[j] = 0, nb[j] = 0;
                if (i < nrec) {
                    const uint32_t r = rec[i];
                    if (r & REC_MATCH) {
                        uint32_t ls, le, lv, ds, de, dv;
                        length_symbol(((r >> 16) & 0xFF) + MIN_MATCH, ls, le, lv);
                        distance_symbol((r & 0xFFFF) + 1, ds, de, dv);
                        const uint32_t lc = S.code[ls], dc = S.code[NLIT + ds];
                        uint32_t b = lc >> 16;
                        v[j] = lc & 0xFFFF;
                        v[j] |= (uint64_t)lv << b, b += le;
                        v[j] |= (uint64_t)(dc & 0xFFFF) << b, b += dc >> 16;
                        v[j] |= (uint64_t)dv << b, b += de;
                        nb[j] = b;
                    } else {
                        const uint32_t c = S.code[r];
                        v[j] = c & 0xFFFF, nb[j] = c >> 16;
                    }
                }
                sum += nb[j];
            }
            uint32_t total;
            uint32_t pos = cb + block_scan256(sum, S.wsum, &total);
#pragma unroll
            for (int j = 0; j < EMIT_ITEMS; ++j) {
                if (nb[j]) {
                    const uint32_t w = pos >> 5, sh = pos & 31;
                    atomicOr(&S.stage[w], (uint32_t)(v[j] << sh));
                    const uint32_t mid = (uint32_t)((v[j] >> 1) >> (31 - sh));
                    if (mid) atomicOr(&S.stage[w + 1], mid);
                    const uint32_t hi = sh ? (uint32_t)((v[j] >> 32) >> (32 - sh)) : 0;
                    if (hi) atomicOr(&S.stage[w + 2], hi);
                    pos += nb[j];
                }
            }
            __syncthreads();
            const uint32_t tot = cb + total, nbytes = tot >> 3;
            const uint8_t *sb = (const uint8_t *)S.stage;
            for (uint32_t x = tid; x < nbytes; x += ENC_THREADS) out[opos + x] = sb[x];
            carry = sb[nbytes];
            cb = tot & 7;
            opos += nbytes;
            __syncthreads();
        }
        if (cb) {
            if (tid == 0) out[opos] = (uint8_t)carry;
            opos += 1;
        }
    }
    if (tid < 4) out[opos + tid] = (uint8_t)(M.crc >> (8 * tid));
    else if (tid < 8) out[opos + tid] = (uint8_t)(n >> (8 * (tid - 4)));
    if (tid == 0) dst_len[s] = (int64_t)opos + 8;
}

// ------------------------------------------------------------------------------------------------
// C entries
// ------------------------------------------------------------------------------------------------
static bool sizes_ok(int64_t nstreams, int64_t total_len) {
    return nstreams >= 0 && nstreams <= RPCC_DEFLATE_MAX_STREAMS && total_len >= 0 && total_len <= MAX_TOTAL;
}

extern "C" size_t rpcc_deflate_bound(int64_t n) { return n < 0 || n > RPCC_DEFLATE_MAX_INPUT ? 0 : (size_t)deflate_bound(n); }

extern "C" size_t rpcc_deflate_workspace_bytes(int64_t nstreams, int64_t total_len) {
    return sizes_ok(nstreams, total_len) ? ws_layout(nstreams, total_len).bytes : 0;
}

extern "C" int rpcc_deflate_encode(const uint64_t *src_ptr, const int64_t *src_len, int64_t nstreams, int64_t total_len, uint8_t *dst,
                                   const int64_t *dst_off, const int64_t *dst_cap, int64_t *dst_len, void *ws, void *stream) {
    ARG_TRY(sizes_ok(nstreams, total_len));
    ARG_TRY(src_ptr && src_len && dst && dst_off && dst_cap && dst_len && ws);
    ARG_TRY(((uintptr_t)ws & 7) == 0);
    if (nstreams == 0) return 0;
    const hipStream_t st = (hipStream_t)stream;
    const WsLayout L = ws_layout(nstreams, total_len);
    StreamMeta *meta = (StreamMeta *)((char *)ws + L.meta);
    uint32_t *recs = (uint32_t *)((char *)ws + L.recs);
    const dim3 grid((unsigned)nstreams);
    hipLaunchKernelGGL(prep_kernel, dim3(1), dim3(1024), 0, st, src_len, dst_cap, nstreams, (int64_t)L.rec_words, meta, dst_len);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(parse_kernel, grid, dim3(ENC_THREADS), 0, st, src_ptr, src_len, meta, recs);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(tables_kernel, grid, dim3(64), 0, st, src_len, dst, dst_off, meta);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(emit_kernel, grid, dim3(ENC_THREADS), 0, st, src_ptr, src_len, dst, dst_off, dst_len, (const StreamMeta *)meta,
                       (const uint32_t *)recs);
    LAUNCH_CHECK();
    return 0;
}
