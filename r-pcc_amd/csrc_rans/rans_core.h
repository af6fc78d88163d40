// rans_core.h -- the 'rans' stream format, versions 1 and 2 (tests/rans_ref.py and tests/rans_filter_ref.py are
// its statements in Python; version 2 is version 1's coded form over filtered bytes, rans_filter.h): the normalisation rule, the parsing of header, tables and directory, and the coding of one chunk by one wavefront.  rans_kernels.hip includes
// it for gfx950 and tests/rans_host_main.cpp for the host; the including file defines how the 64 lanes are spoken to:
//   RANS_FN             function qualifiers
//   RANS_NL             lanes one thread of control carries: 1 on the device (the hardware runs the 64), 64 on the host
//   RANS_EACH(l)        loop header over the lanes this thread carries; l is the lane's number, 0 .. 63
//   RANS_AT(a, l)       the element of a per-lane array a (declared T a[RANS_NL]) that belongs to lane l
//   RANS_BALLOT(a)      64-bit mask of the lanes whose a is not 0          RANS_SUM64(a)   sum of a (uint64_t) over the 64 lanes
//   RANS_MAX32(a)       maximum of a (uint32_t) over the 64 lanes          RANS_SYNC()     the wave's stores to `ring` are visible to its loads
// A per-lane loop body never reads another lane's variables: what the lanes tell each other goes through the four collectives and the
// word ring only, so the host's lane-after-lane order and the device's lockstep give the same bytes.
#ifndef RPCC_RANS_CORE_H
#define RPCC_RANS_CORE_H

#include <stdint.h>
#include <string.h>

#define RANS_HEADER 12
#define RANS_PROB_BITS 12
#define RANS_PROB 4096u
#define RANS_LOW 65536u          // the encoder's start state and the decoder's end state; states live in [2^16, 2^32)
#define RANS_LANES 64
#define RANS_RING 2048           // uint16 words of a wave's payload ring, kept as RANS_RING / 2 dwords (a round takes at most 64 words)
#define RANS_FILL (RANS_RING / 2 / (2 * RANS_LANES))   // dwords a lane loads when half the ring is topped up
#define RANS_MIN_CHUNK_LOG2 8
#define RANS_MAX_CHUNK_LOG2 16
#define RANS_ENC_BLOCK 8         // rounds whose input bytes the encoder loads ahead

RANS_FN uint32_t rans_ld16(const uint8_t *p) {
    uint16_t v;
    __builtin_memcpy(&v, p, 2);
    return v;
}
RANS_FN uint32_t rans_ld32(const uint8_t *p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}
RANS_FN void rans_st16(uint8_t *p, uint32_t v) {
    const uint16_t w = (uint16_t)v;
    __builtin_memcpy(p, &w, 2);
}
RANS_FN void rans_st32(uint8_t *p, uint32_t v) { __builtin_memcpy(p, &v, 4); }

#include "rans_filter.h"

RANS_FN void rans_put_header(uint8_t *o, uint32_t mode, uint32_t width, uint32_t n, uint32_t chunk_log2) {
    o[0] = 'R', o[1] = 'A', o[2] = (uint8_t)mode, o[3] = (uint8_t)width;
    rans_st32(o + 4, n);
    o[8] = (uint8_t)chunk_log2, o[9] = 0, o[10] = 0, o[11] = 0;
}
// The version-2 header: magic 'R' 'B', always coded (mode 1), the filter in byte 9.
RANS_FN void rans_put_header_filtered(uint8_t *o, uint32_t width, uint32_t n, uint32_t chunk_log2, uint32_t filter) {
    rans_put_header(o, 1, width, n, chunk_log2);
    o[1] = 'B', o[9] = (uint8_t)filter;
}

// Bytes of plane p in a stream of n bytes.
RANS_FN uint32_t rans_plane_bytes(uint32_t n, uint32_t width, uint32_t p) { return n > p ? (n - p + width - 1) / width : 0; }

// ------------------------------------------------------------------------------------------------
// exact division by a frequency
// ------------------------------------------------------------------------------------------------
// floor(x / f) for every 32-bit x and f in 1 .. 4096 (Granlund & Montgomery 1994, figure 4.1 at N = 32): with l = ceil(log2 f) and
// m = floor(2^32 (2^l - f) / f) + 1, t = mulhi(m, x) and q = (t + ((x - t) >> min(l, 1))) >> max(l - 1, 0).  m + 2^32 is
// ceil(2^(32+l) / f) up to the rounding the theorem allows: 2^(32+l) <= (m + 2^32) f <= 2^(32+l) + 2^l, which gives floor(x / f) for all
// x < 2^32; t <= x, so x - t does not wrap, and t + ((x - t) >> 1) <= x does not overflow.  DESIGN.md section 19 has the argument in
// full; tests/rans_host_main.cpp checks every f at the boundary states.
RANS_FN uint32_t rans_log2_ceil(uint32_t f) {
    uint32_t l = 0;
    while ((1u << l) < f) ++l;
    return l;
}
RANS_FN uint32_t rans_rcp(uint32_t f) {
    const uint32_t l = rans_log2_ceil(f);
    return (uint32_t)((((uint64_t)((1u << l) - f)) << 32) / f) + 1u;
}
RANS_FN uint32_t rans_div(uint32_t x, uint32_t m, uint32_t l) {
    const uint32_t t = (uint32_t)(((uint64_t)m * x) >> 32);
    return (t + ((x - t) >> (l ? 1 : 0))) >> (l ? l - 1 : 0);
}
// The encoder's table entry of a symbol: word 0 the reciprocal, word 1 = f | cum << 13 | l << 25.
RANS_FN void rans_enc_entry(uint32_t f, uint32_t cum, uint32_t *e) {
    e[0] = rans_rcp(f);
    e[1] = f | cum << 13 | rans_log2_ceil(f) << 25;
}
// The decoder's table entry of a symbol: (f - 1) | cum << 16.
RANS_FN uint32_t rans_dec_entry(uint32_t f, uint32_t cum) { return (f - 1) | cum << 16; }

// ------------------------------------------------------------------------------------------------
// normalisation
// ------------------------------------------------------------------------------------------------
// counts[256] of one plane, total their sum (> 0) -> freq[256] summing to 4096, 0 exactly where the count is 0.  Lane l holds symbols
// 4 l .. 4 l + 3.  f = max(1, floor(count * 4096 / total)); a remainder goes to the symbol with the largest f, the lowest such symbol; a
// deficit is taken back one at a time, each from the symbol with the largest f at that moment, the lowest such symbol.
RANS_FN void rans_normalise(const int lane, const uint32_t *counts, const uint64_t total, uint16_t *freq) {
    (void)lane;
    uint32_t f[RANS_NL][4], key[RANS_NL];
    uint64_t part[RANS_NL];
    RANS_EACH(l) {
        uint64_t s = 0;
        for (int j = 0; j < 4; ++j) {
            const uint64_t c = counts[4 * l + j];
            const uint32_t v = c ? (uint32_t)(c * RANS_PROB / total) : 0;
            RANS_AT(f, l)[j] = c && !v ? 1 : v;
            s += RANS_AT(f, l)[j];
        }
        RANS_AT(part, l) = s;
    }
    const uint32_t sum = (uint32_t)RANS_SUM64(part);
    const uint32_t steps = sum <= RANS_PROB ? 1 : sum - RANS_PROB;
    for (uint32_t it = 0; it < steps; ++it) {
        RANS_EACH(l) {
            uint32_t k = 0;
            for (int j = 0; j < 4; ++j) {
                const uint32_t kj = RANS_AT(f, l)[j] << 8 | (255u - (uint32_t)(4 * l + j));
                k = kj > k ? kj : k;
            }
            RANS_AT(key, l) = k;
        }
        const uint32_t best = RANS_MAX32(key);
        RANS_EACH(l) {
            for (int j = 0; j < 4; ++j)
                if ((RANS_AT(f, l)[j] << 8 | (255u - (uint32_t)(4 * l + j))) == best) {
                    if (sum <= RANS_PROB) RANS_AT(f, l)[j] += RANS_PROB - sum;
                    else RANS_AT(f, l)[j] -= 1;
                }
        }
    }
    RANS_EACH(l) {
        for (int j = 0; j < 4; ++j) freq[4 * l + j] = (uint16_t)RANS_AT(f, l)[j];
    }
}

// ------------------------------------------------------------------------------------------------
// header, tables, directory
// ------------------------------------------------------------------------------------------------
struct RansInfo {
    uint32_t mode, width, n, chunk_log2, nch;
    uint32_t filter;        // RANS_FILTER_*: 0 for every 'RA' stream
    uint32_t m[4];          // symbols of each plane's table
    int64_t tab[4];         // where each plane's entries start
    int64_t dir, pay;       // where the directory and the first payload start
};

// What the first 12 bytes say, unchecked but for the length; every lane reads the same.  -> false when there are fewer than 12.
RANS_FN bool rans_read_header(const uint8_t *in, int64_t len, RansInfo &I) {
    if (len < RANS_HEADER) return false;
    I.mode = in[2], I.width = in[3], I.n = rans_ld32(in + 4), I.chunk_log2 = in[8];
    I.filter = in[1] == 'B' ? in[9] : RANS_FILTER_NONE;
    return true;
}

// The validation pass of one stream by one wave: every rule of the format short of decoding the chunks.  -> RPCC_RANS_OK or E_*.
RANS_FN int rans_parse(const int lane, const uint8_t *in, const int64_t len, const int64_t cap, RansInfo &I) {
    (void)lane;
    if (!rans_read_header(in, len, I)) return RPCC_RANS_E_TRUNCATED;
    // 'RA': byte 9 is reserved; 'RB': byte 9 is the filter and must be 1, and the stream is coded (there is no stored form)
    const bool v2 = in[1] == 'B';
    if (in[0] != 'R' || (in[1] != 'A' && !v2) || I.mode > 1 || (v2 && (I.mode != 1 || in[9] != RANS_FILTER_DELTA)) || !(I.width == 1 || I.width == 2 || I.width == 4) || I.chunk_log2 < RANS_MIN_CHUNK_LOG2 ||
        I.chunk_log2 > RANS_MAX_CHUNK_LOG2 || (!v2 && in[9]) || in[10] || in[11] || I.n > RPCC_RANS_MAX_INPUT || (I.mode == 1 && I.n == 0))
        return RPCC_RANS_E_HEADER;
    if ((int64_t)I.n > cap) return RPCC_RANS_E_CAPACITY;
    I.nch = 0;
    if (I.mode == 0) return len == RANS_HEADER + (int64_t)I.n ? RPCC_RANS_OK : RPCC_RANS_E_DIRECTORY;
    int64_t pos = RANS_HEADER;
#pragma unroll
    for (uint32_t p = 0; p < 4; ++p) {   // (unrolled: I.m / I.tab stay in registers)
        if (p >= I.width) break;
        if (pos + 2 > len) return RPCC_RANS_E_TRUNCATED;
        const uint32_t m = rans_ld16(in + pos);
        pos += 2;
        if (m > 256 || (m == 0) != (I.n <= p)) return RPCC_RANS_E_TABLE;
        if (pos + 3 * (int64_t)m > len) return RPCC_RANS_E_TRUNCATED;
        I.m[p] = m, I.tab[p] = pos;
        uint64_t sum[RANS_NL];
        int bad[RANS_NL];
        RANS_EACH(l) {
            uint64_t s = 0;
            int b = 0;
            for (uint32_t e = (uint32_t)l; e < m; e += RANS_LANES) {
                const uint8_t *q = in + pos + 3 * (int64_t)e;
                const uint32_t fm1 = rans_ld16(q + 1);
                b |= fm1 >= RANS_PROB || (e > 0 && q[-3] >= q[0]);
                s += fm1 + 1;
            }
            RANS_AT(sum, l) = s, RANS_AT(bad, l) = b;
        }
        if (RANS_BALLOT(bad)) return RPCC_RANS_E_TABLE;
        if (m && RANS_SUM64(sum) != RANS_PROB) return RPCC_RANS_E_TABLE;
        pos += 3 * (int64_t)m;
    }
    I.nch = (uint32_t)(((uint64_t)I.n + (1u << I.chunk_log2) - 1) >> I.chunk_log2);
    if (pos + 4 * (int64_t)I.nch > len) return RPCC_RANS_E_TRUNCATED;
    I.dir = pos;
    pos += 4 * (int64_t)I.nch;
    I.pay = pos;
    uint64_t sum[RANS_NL];
    RANS_EACH(l) {
        uint64_t s = 0;
        for (uint32_t c = (uint32_t)l; c < I.nch; c += RANS_LANES) s += rans_ld32(in + I.dir + 4 * (int64_t)c);
        RANS_AT(sum, l) = s;
    }
    return RANS_SUM64(sum) == (uint64_t)(len - pos) ? RPCC_RANS_OK : RPCC_RANS_E_DIRECTORY;
}

// Where the tables, the directory and the payloads of a coded stream lie, for a stream rans_parse has accepted (nothing is checked again).
RANS_FN void rans_layout(const uint8_t *in, RansInfo &I) {
    int64_t pos = RANS_HEADER;
#pragma unroll
    for (uint32_t p = 0; p < 4; ++p) {   // (unrolled: I.m / I.tab stay in registers)
        if (p >= I.width) break;
        I.m[p] = rans_ld16(in + pos);
        I.tab[p] = pos + 2;
        pos += 2 + 3 * (int64_t)I.m[p];
    }
    I.nch = (uint32_t)(((uint64_t)I.n + (1u << I.chunk_log2) - 1) >> I.chunk_log2);
    I.dir = pos;
    I.pay = pos + 4 * (int64_t)I.nch;
}

// The payload offset of chunk c: the sum of the directory's entries before it.
RANS_FN int64_t rans_chunk_offset(const int lane, const uint8_t *in, const RansInfo &I, const uint32_t c) {
    (void)lane;
    uint64_t sum[RANS_NL];
    RANS_EACH(l) {
        uint64_t s = 0;
        for (uint32_t e = (uint32_t)l; e < c; e += RANS_LANES) s += rans_ld32(in + I.dir + 4 * (int64_t)e);
        RANS_AT(sum, l) = s;
    }
    return I.pay + (int64_t)RANS_SUM64(sum);
}

// ------------------------------------------------------------------------------------------------
// one chunk by one wave
// ------------------------------------------------------------------------------------------------
// Decodes the k bytes of a chunk from its payload.  lookup: [width][4096] slot -> symbol; fc: [width][256] rans_dec_entry; ring: RANS_RING / 2
// dwords of the wave's own.  out: the chunk's place in the output, or null to check the chunk and write nothing.
RANS_FN int rans_decode_chunk(const int lane, const uint8_t *pay, const uint32_t plen, const uint32_t k, const uint32_t width,
                              const uint8_t *lookup, const uint32_t *fc, uint32_t *ring, uint8_t *out) {
    (void)lane;
    const uint32_t L = k < RANS_LANES ? k : RANS_LANES;
    if (plen < 4 * L || ((plen - 4 * L) & 1)) return RPCC_RANS_E_PAYLOAD;
    const uint32_t nw = (plen - 4 * L) / 2;
    const uint8_t *words = pay + 4 * L;
    uint32_t x[RANS_NL], sym[RANS_NL];
    int need[RANS_NL];
    RANS_EACH(l) { RANS_AT(x, l) = (uint32_t)l < L ? rans_ld32(pay + 4 * l) : RANS_LOW; }
    uint32_t filled = 0, pos = 0;
    for (uint32_t r = 0; r * RANS_LANES < k; ++r) {
        if (filled < nw && pos + RANS_LANES > filled) {   // the slots of [filled, top) held words before pos: top - RANS_RING <= filled - RANS_RING / 2 < pos
            const uint32_t top = nw - filled < RANS_RING / 2 ? nw : filled + RANS_RING / 2;
            const uint32_t np = (top - filled) >> 1;      // filled is even: whole word pairs as dwords, an odd last word on its own
            RANS_EACH(l) {                                // all of a lane's loads, free of branches (a pair beyond the last reads the last again), then its stores
                uint32_t v[RANS_FILL];
#pragma unroll
                for (uint32_t j = 0; j < RANS_FILL; ++j) {
                    const uint32_t q = (uint32_t)l + RANS_LANES * j;
                    v[j] = np ? rans_ld32(words + 2 * (int64_t)filled + 4 * (int64_t)(q < np ? q : np - 1)) : 0;
                }
#pragma unroll
                for (uint32_t j = 0; j < RANS_FILL; ++j) {
                    const uint32_t q = (uint32_t)l + RANS_LANES * j;
                    if (q < np) ring[((filled & (RANS_RING - 1)) >> 1) + q] = v[j];
                }
                if (l == 0 && ((top - filled) & 1)) ring[((top - 1) & (RANS_RING - 1)) >> 1] = rans_ld16(words + 2 * (int64_t)(top - 1));
            }
            filled = top;
            RANS_SYNC();
        }
        RANS_EACH(l) {
            const uint32_t i = r * RANS_LANES + (uint32_t)l;
            RANS_AT(need, l) = 0;
            if (i < k) {
                const uint32_t p = (uint32_t)l & (width - 1), v = RANS_AT(x, l), slot = v & (RANS_PROB - 1);
                const uint32_t s = lookup[p * RANS_PROB + slot], e = fc[p * 256 + s];
                const uint32_t y = ((e & 0xFFFu) + 1) * (v >> RANS_PROB_BITS) + slot - (e >> 16);
                RANS_AT(x, l) = y, RANS_AT(sym, l) = s, RANS_AT(need, l) = y < RANS_LOW;
            }
        }
        const uint64_t mask = RANS_BALLOT(need);
        const uint32_t cnt = (uint32_t)__builtin_popcountll(mask);
        if (cnt > nw - pos) return RPCC_RANS_E_PAYLOAD;
        RANS_EACH(l) {
            const uint32_t i = r * RANS_LANES + (uint32_t)l;
            if (RANS_AT(need, l)) {
                const uint32_t rank = (uint32_t)__builtin_popcountll(mask & ((1ull << l) - 1ull));
                const uint32_t w = (pos + rank) & (RANS_RING - 1);
                RANS_AT(x, l) = RANS_AT(x, l) << 16 | ((ring[w >> 1] >> (16 * (w & 1))) & 0xFFFFu);
            }
            if (out && i < k) out[i] = (uint8_t)RANS_AT(sym, l);
        }
        pos += cnt;
    }
    RANS_EACH(l) { RANS_AT(need, l) = (uint32_t)l < L && RANS_AT(x, l) != RANS_LOW; }
    return RANS_BALLOT(need) || pos != nw ? RPCC_RANS_E_STATE : RPCC_RANS_OK;
}

// Codes the k bytes at src into the payload that ends at slot_end (the words are written backwards from there, the states in front of
// them once their count is known; at most 2 k + 256 bytes).  enc: [width][256][2] rans_enc_entry.  filter (the same in every lane):
// RANS_FILTER_DELTA reads the bytes through the forward filter as they are loaded.  -> the payload's length.
RANS_FN uint32_t rans_encode_chunk_filtered(const int lane, const uint8_t *src, const uint32_t k, const uint32_t width, const uint32_t filter,
                                            const uint32_t *enc, uint8_t *slot_end) {
    (void)lane;
    const uint32_t L = k < RANS_LANES ? k : RANS_LANES, R = (k + RANS_LANES - 1) / RANS_LANES;
    uint32_t x[RANS_NL], wv[RANS_NL];
    int emit[RANS_NL];
    uint8_t b[RANS_NL][RANS_ENC_BLOCK];
    RANS_EACH(l) { RANS_AT(x, l) = RANS_LOW; }
    uint32_t total = 0;
    for (uint32_t r1 = R; r1 > 0;) {           // rounds [r0, r1), last to first; r0 a multiple of RANS_ENC_BLOCK
        const uint32_t r0 = (r1 - 1) / RANS_ENC_BLOCK * RANS_ENC_BLOCK;
        if (filter == RANS_FILTER_NONE) {
            RANS_EACH(l) {
#pragma unroll
                for (uint32_t j = 0; j < RANS_ENC_BLOCK; ++j) {
                    const uint32_t i = (r0 + j) * RANS_LANES + (uint32_t)l;
                    RANS_AT(b, l)[j] = i < k ? src[i] : 0;
                }
            }
        } else if (r0 > 0 && (r0 + RANS_ENC_BLOCK) * RANS_LANES <= k - (k & (width - 1))) {
            // every byte of the block in a whole element behind the chunk's first: loads without conditions, the width a literal
#define RANS_DELTA_BLOCK(W)                                                                              \
    RANS_EACH(l) {                                                                                       \
        _Pragma("unroll") for (uint32_t j = 0; j < RANS_ENC_BLOCK; ++j)                                  \
            RANS_AT(b, l)[j] = (uint8_t)rans_delta_byte_inner(src, (r0 + j) * RANS_LANES + (uint32_t)l, W); \
    }
            if (width == 2) RANS_DELTA_BLOCK(2)
            else if (width == 4) RANS_DELTA_BLOCK(4)
            else RANS_DELTA_BLOCK(1)
#undef RANS_DELTA_BLOCK
        } else {                                      // the chunk's first block and its last
            RANS_EACH(l) {
#pragma unroll
                for (uint32_t j = 0; j < RANS_ENC_BLOCK; ++j) {
                    const uint32_t i = (r0 + j) * RANS_LANES + (uint32_t)l;
                    RANS_AT(b, l)[j] = i < k ? (uint8_t)rans_delta_byte(src, i, k, width) : 0;
                }
            }
        }
#pragma unroll
        for (uint32_t j = RANS_ENC_BLOCK; j-- > 0;) {
            const uint32_t r = r0 + j;
            if (r >= r1) continue;
            RANS_EACH(l) {
                RANS_AT(emit, l) = 0;
                if (r * RANS_LANES + (uint32_t)l < k) {
                    const uint32_t *e = enc + (((uint32_t)l & (width - 1)) * 256 + RANS_AT(b, l)[j]) * 2;
                    const uint32_t f = e[1] & 0x1FFFu, c = (e[1] >> 13) & 0xFFFu;
                    uint32_t v = RANS_AT(x, l);
                    if ((v >> 20) >= f) {        // v >= f << 20
                        RANS_AT(emit, l) = 1, RANS_AT(wv, l) = v & 0xFFFFu;
                        v >>= 16;
                    }
                    const uint32_t q = rans_div(v, e[0], e[1] >> 25);
                    RANS_AT(x, l) = (q << RANS_PROB_BITS) + (v - q * f) + c;
                }
            }
            const uint64_t mask = RANS_BALLOT(emit);
            RANS_EACH(l) {
                if (RANS_AT(emit, l)) {          // the decoder's lanes take a round's words in ascending order: the highest lane is emitted first
                    const uint32_t rank = (uint32_t)__builtin_popcountll((mask >> l) >> 1);
                    rans_st16(slot_end - 2 * (int64_t)(total + rank + 1), RANS_AT(wv, l));
                }
            }
            total += (uint32_t)__builtin_popcountll(mask);
        }
        r1 = r0;
    }
    RANS_EACH(l) {
        if ((uint32_t)l < L) rans_st32(slot_end - 2 * (int64_t)total - 4 * (int64_t)L + 4 * l, RANS_AT(x, l));
    }
    return 4 * L + 2 * total;
}
RANS_FN uint32_t rans_encode_chunk(const int lane, const uint8_t *src, const uint32_t k, const uint32_t width, const uint32_t *enc, uint8_t *slot_end) {
    return rans_encode_chunk_filtered(lane, src, k, width, RANS_FILTER_NONE, enc, slot_end);
}

#endif  // RPCC_RANS_CORE_H
