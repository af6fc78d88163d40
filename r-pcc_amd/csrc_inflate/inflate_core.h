// inflate_core.h -- the decoder of one gzip member by one wavefront (tests/inflate_ref.py is its statement in
// Python).  inflate_kernels.hip includes it for gfx950; the including file defines how the wave is spoken to:
//   INF_FN            function qualifiers            INF_CONST         qualifiers of a constant table
//   INF_WAVE          lanes per wave                 INF_SYNC()        barrier of the wave's LDS traffic
//   INF_UNI(x)        x, known to be equal in every lane, as a scalar (int)
//   INF_BALLOT(p)     64-bit mask of the lanes where p holds            INF_SHFL_XOR(v, m)  v of lane ^ m
//   INF_BREV(x)       the 32 bits of x in reverse order
// With INF_WAVE 1 and empty INF_SYNC the same text is an ordinary sequential inflate.
//
// Everything the symbol loop decides is equal in all lanes (bit buffer, positions, status); the lanes part only to build tables, to copy
// and to fold the CRC.  Output goes to the LDS ring first; pieces of INF_FLUSH bytes leave it for global memory with their CRC folded on
// the way, so a match is served from the ring and the wave never reads back what it stored.
#ifndef RPCC_INFLATE_CORE_H
#define RPCC_INFLATE_CORE_H

#include <stdint.h>

#define INF_RING 32768          // the deflate window: output position x at ring[x & (INF_RING - 1)]
#define INF_WIN 2048            // bytes of the input window
#define INF_FLUSH (65 * 64)     // bytes of a piece: 65 per lane, an odd stride in bytes between the lanes' CRC chunks
#define INF_LIT_ROOT 10         // first-level bits of the literal/length table; longer codes are read bit by bit
#define INF_DIST_ROOT 8
#define INF_CL_ROOT 7           // the code-length code has no longer codes
#define INF_CODES 0
#define INF_LENS 1
#define INF_DISTS 2
static_assert(INF_FLUSH + 258 < INF_RING / 2, "a piece and a match must fit in the ring beside the bytes not yet flushed");

struct InfShared {
    uint8_t ring[INF_RING];
    uint8_t win[INF_WIN];                   // input bytes [wb, wb + INF_WIN)
    uint16_t lit[1 << INF_LIT_ROOT];        // symbol | length << 9 at every index whose low `length` bits are the code; 0: none
    uint16_t dist[1 << INF_DIST_ROOT];
    uint16_t cl[1 << INF_CL_ROOT];
    uint16_t sorted[2][288];                // symbols by (length, symbol): [0] literal/length, [1] distance
    uint16_t cnt[2][16];                    // codes per length
    uint32_t crc_tab[256];
    uint8_t lens[320];                      // code lengths: 19 of the code-length code, then HLIT + HDIST (288 + 32 in a fixed block)
};

INF_CONST uint16_t INF_LEN_BASE[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
INF_CONST uint8_t INF_LEN_EXTRA[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
INF_CONST uint16_t INF_DIST_BASE[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
                                        8193, 12289, 16385, 24577};
INF_CONST uint8_t INF_DIST_EXTRA[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
INF_CONST uint8_t INF_CL_ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// a * b in GF(2)[x] modulo the CRC-32 polynomial, bit-reflected as the CRC register is (x^0 = 0x80000000)
INF_FN uint32_t inf_gf_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 31; i >= 0; --i) {
        p ^= b & (0u - ((a >> i) & 1u));
        b = (b >> 1) ^ (0xEDB88320u & (0u - (b & 1u)));
    }
    return p;
}

// x^(8 * bytes): what a CRC register is multiplied by when `bytes` more bytes follow
INF_FN uint32_t inf_gf_pow8(uint32_t bytes) {
    uint32_t p = 0x80000000u, base = 0x00800000u;
    for (; bytes; bytes >>= 1) {
        if (bytes & 1u) p = inf_gf_mul(p, base);
        base = inf_gf_mul(base, base);
    }
    return p;
}

// The decode table of n code lengths (zlib's rules: over-subscribed is an error; incomplete is one for the code-length code, and for the
// others unless the only code has length 1 -- or, for distances, there is none).  Every lane takes symbols lane, lane + INF_WAVE, ...; a
// symbol's rank among those of its length comes from ballots.  -> 0 or RPCC_INFLATE_E_TABLE
INF_FN int inf_build_table(const int lane, const uint8_t *lens, const int n, uint16_t *table, const int root, uint16_t *sorted, uint16_t *cnt_out,
                           const int kind) {
    int cnt[16], first[16], offs[16];
#pragma unroll
    for (int b = 0; b < 16; ++b) cnt[b] = 0;
    for (int s0 = 0; s0 < n; s0 += INF_WAVE) {
        const int s = s0 + lane, L = s < n ? lens[s] : 0;
#pragma unroll
        for (int b = 1; b < 16; ++b) cnt[b] += __builtin_popcountll(INF_BALLOT(L == b));
    }
    int left = 1, mx = 0, code = 0, o = 0;
#pragma unroll
    for (int b = 1; b < 16; ++b) {
        left = 2 * left - cnt[b];
        if (left < 0) return RPCC_INFLATE_E_TABLE;
        if (cnt[b]) mx = b;
        code = (code + cnt[b - 1]) << 1;
        first[b] = code;
        offs[b] = o;
        o += cnt[b];
    }
    if (left > 0 && (kind == INF_CODES || mx > 1 || (mx == 0 && kind != INF_DISTS))) return RPCC_INFLATE_E_TABLE;
    for (int x = lane; x < (1 << root); x += INF_WAVE) table[x] = 0;
    if (cnt_out && lane == 0) {
#pragma unroll
        for (int b = 1; b < 16; ++b) cnt_out[b] = (uint16_t)cnt[b];
    }
    INF_SYNC();
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int s0 = 0; s0 < n; s0 += INF_WAVE) {
        const int s = s0 + lane, L = s < n ? lens[s] : 0;
        uint32_t c = 0, idx = 0;
#pragma unroll
        for (int b = 1; b < 16; ++b) {
            const unsigned long long m = INF_BALLOT(L == b);
            if (L == b) {
                const int r = __builtin_popcountll(m & below);
                c = (uint32_t)(first[b] + r);
                idx = (uint32_t)(offs[b] + r);
            }
            const int p = __builtin_popcountll(m);
            first[b] += p;
            offs[b] += p;
        }
        if (L) {
            if (sorted) sorted[idx] = (uint16_t)s;
            if (L <= root) {
                const uint16_t e = (uint16_t)(s | L << 9);
                for (uint32_t x = INF_BREV(c) >> (32 - L); x < (1u << root); x += 1u << L) table[x] = e;
            }
        }
    }
    INF_SYNC();
    return 0;
}

#define INF_FAIL(code)  \
    do {                \
        op_out = op;    \
        return (code);  \
    } while (0)

// One stream: in[0, iend) -> out[0, cap).  -> status; op_out = bytes produced.
INF_FN int inflate_stream(InfShared &S, const int lane, const uint8_t *__restrict__ in, const int64_t iend, uint8_t *__restrict__ out,
                          const int64_t cap, int64_t &op_out) {
    int64_t op = 0, flushed = 0;
    if (iend <= 0) INF_FAIL(iend == 0 ? RPCC_INFLATE_OK : RPCC_INFLATE_E_TRUNCATED);
    for (int i = lane; i < 256; i += INF_WAVE) {
        uint32_t r = (uint32_t)i;
        for (int k = 0; k < 8; ++k) r = (r >> 1) ^ (0xEDB88320u & (0u - (r & 1u)));
        S.crc_tab[i] = r;
    }
    uint32_t crc = 0xFFFFFFFFu;      // the register over out[0, flushed)
    int64_t wb = -INF_WIN;           // window base: empty
    // one input byte at 0 <= ip < iend, through the window (every lane asks for the same ip)
    auto get = [&](int64_t ip) -> uint32_t {
        if (ip < wb || ip >= wb + INF_WIN) {
            INF_SYNC();
            wb = ip;
            for (int64_t x = lane; x < INF_WIN && wb + x < iend; x += INF_WAVE) S.win[x] = in[wb + x];
            INF_SYNC();
        }
        return (uint32_t)INF_UNI(S.win[ip - wb]);
    };
    int64_t ip = 0;                  // the next input byte that enters the bit buffer
    uint64_t bb = 0;                 // bc valid bits, zero above them
    int bc = 0;
    auto refill = [&]() {            // bc < 57 on entry where it matters; brings bc to 56 or more, or to all that is left
        if (bc < 56 && ip >= wb && ip + 8 <= wb + INF_WIN && ip + 8 <= iend) {   // eight window bytes in one round trip, the whole ones kept
            const uint8_t *w = S.win + (ip - wb);
            const uint32_t lo = (uint32_t)w[0] | (uint32_t)w[1] << 8 | (uint32_t)w[2] << 16 | (uint32_t)w[3] << 24;
            const uint32_t hi = (uint32_t)w[4] | (uint32_t)w[5] << 8 | (uint32_t)w[6] << 16 | (uint32_t)w[7] << 24;
            const int nb = (63 - bc) >> 3;   // 1 .. 7 bytes fit
            const uint64_t v = ((uint64_t)(uint32_t)INF_UNI(hi) << 32 | (uint32_t)INF_UNI(lo)) & ((1ull << (8 * nb)) - 1ull);
            bb |= v << bc;
            bc += 8 * nb;
            ip += nb;
            return;
        }
        while (bc <= 56 && ip < iend) {
            bb |= (uint64_t)get(ip) << bc;
            bc += 8;
            ++ip;
        }
    };
    auto take = [&](int n, uint32_t &v) -> bool {   // n <= 16 bits; false: the input ends first
        if (bc < n) {
            refill();
            if (bc < n) return false;
        }
        v = (uint32_t)bb & ((1u << n) - 1u);
        bb >>= n;
        bc -= n;
        return true;
    };
    auto to_byte = [&]() {           // drop the rest of the current byte and hand the buffered bytes back
        bb >>= bc & 7;
        bc -= bc & 7;
        ip -= bc >> 3;
        bb = 0;
        bc = 0;
    };
    // one symbol of table t (0 literal/length, 1 distance; -1 the code-length code) -> 0 or a status
    auto symbol = [&](int t, const uint16_t *table, int root, uint32_t &sym) -> int {
        if (bc < 15) refill();
        const uint32_t e = (uint32_t)INF_UNI(table[(uint32_t)bb & ((1u << root) - 1u)]);
        if (e) {
            const int L = (int)(e >> 9);
            if (L > bc) return RPCC_INFLATE_E_TRUNCATED;
            sym = e & 511u;
            bb >>= L;
            bc -= L;
            return 0;
        }
        if (t < 0) return RPCC_INFLATE_E_SYMBOL;
        int code = 0, first = 0, index = 0;
        for (int b = 1; b <= 15; ++b) {
            if (bc < b) return RPCC_INFLATE_E_TRUNCATED;
            code |= (int)((bb >> (b - 1)) & 1u);
            const int c = INF_UNI(S.cnt[t][b]);
            if (code - c < first) {
                sym = (uint32_t)INF_UNI(S.sorted[t][index + code - first]);
                bb >>= b;
                bc -= b;
                return 0;
            }
            index += c;
            first = (first + c) << 1;
            code <<= 1;
        }
        return RPCC_INFLATE_E_SYMBOL;
    };
    // out[flushed, flushed + n) leaves the ring (n > 0, the ring's stores done): coalesced stores, and the CRC.  Lane l folds c = ceil(n / wave)
    // bytes of the piece, laid out so that it ENDS with the last lane: the lanes before the piece's first byte hold a zero register,
    // which stays zero; the lane of the first byte starts from the running register.  reg(A ++ B) = reg(A) * x^(8|B|) + reg0(B).
    auto flush = [&](int64_t n) {
        for (int64_t x = lane; x < n; x += INF_WAVE) out[flushed + x] = S.ring[(flushed + x) & (INF_RING - 1)];
        const int64_t c = (n + INF_WAVE - 1) / INF_WAVE, pad = c * INF_WAVE - n;
        int64_t a = lane * c - pad;
        const int64_t b = a + c;
        uint32_t r = 0;
        if (b > 0) {
            if (a <= 0) {
                a = 0;
                r = crc;
            }
            for (int64_t x = a; x < b; ++x) r = S.crc_tab[(r ^ S.ring[(flushed + x) & (INF_RING - 1)]) & 255u] ^ (r >> 8);
        }
        uint32_t m = inf_gf_pow8((uint32_t)c);
        for (int k = 1; k < INF_WAVE; k <<= 1) {
            if (!(lane & k)) r = inf_gf_mul(r, m);
            r ^= INF_SHFL_XOR(r, k);
            m = inf_gf_mul(m, m);
        }
        crc = r;
        flushed += n;
        INF_SYNC();
    };

    // ---- the member's header, as Python's gzip reads it
    if (iend < 2) INF_FAIL(RPCC_INFLATE_E_TRUNCATED);
    if (get(0) != 0x1Fu || get(1) != 0x8Bu) INF_FAIL(RPCC_INFLATE_E_HEADER);
    if (iend < 3) INF_FAIL(RPCC_INFLATE_E_TRUNCATED);
    if (get(2) != 8u) INF_FAIL(RPCC_INFLATE_E_HEADER);
    if (iend < 10) INF_FAIL(RPCC_INFLATE_E_TRUNCATED);
    const uint32_t flg = get(3);
    ip = 10;
    if (flg & 4u) {                                    // FEXTRA
        if (iend - ip < 2) INF_FAIL(RPCC_INFLATE_E_TRUNCATED);
        const int64_t xlen = (int64_t)(get(ip) | get(ip + 1) << 8);
        ip += 2;
        if (iend - ip < xlen) INF_FAIL(RPCC_INFLATE_E_TRUNCATED);
        ip += xlen;
    }
    for (uint32_t bit = 8u; bit <= 16u; bit <<= 1) {   // FNAME, FCOMMENT
        if (flg & bit) {
            uint32_t ch;
            do {
                if (ip >= iend) INF_FAIL(RPCC_INFLATE_E_TRUNCATED);
                ch = get(ip++);
            } while (ch);
        }
    }
    if (flg & 2u) {                                    // FHCRC
        if (iend - ip < 2) INF_FAIL(RPCC_INFLATE_E_TRUNCATED);
        ip += 2;
    }

    // ---- the blocks
    for (;;) {
        uint32_t final_, btype;
        if (!take(1, final_) || !take(2, btype)) INF_FAIL(RPCC_INFLATE_E_TRUNCATED);
        if (btype == 3u) INF_FAIL(RPCC_INFLATE_E_BTYPE);
        if (btype == 0u) {
            to_byte();
            if (iend - ip < 4) INF_FAIL(RPCC_INFLATE_E_TRUNCATED);
            const uint32_t len = get(ip) | get(ip + 1) << 8, nlen = get(ip + 2) | get(ip + 3) << 8;
            ip += 4;
            if (len != (~nlen & 0xFFFFu)) INF_FAIL(RPCC_INFLATE_E_STORED);
            if ((int64_t)len > iend - ip) INF_FAIL(RPCC_INFLATE_E_TRUNCATED);
            if ((int64_t)len > cap - op) INF_FAIL(RPCC_INFLATE_E_OVERRUN);
            for (int64_t rest = len; rest > 0;) {
                const int64_t piece = rest < INF_FLUSH ? rest : INF_FLUSH;
                for (int64_t x = lane; x < piece; x += INF_WAVE) S.ring[(op + x) & (INF_RING - 1)] = in[ip + x];
                op += piece;
                ip += piece;
                rest -= piece;
                INF_SYNC();
                while (op - flushed >= INF_FLUSH) flush(INF_FLUSH);
            }
        } else {
            if (btype == 1u) {
                for (int x = lane; x < 320; x += INF_WAVE) S.lens[x] = (uint8_t)(x < 144 ? 8 : x < 256 ? 9 : x < 280 ? 7 : x < 288 ? 8 : 5);
                INF_SYNC();
                inf_build_table(lane, S.lens, 288, S.lit, INF_LIT_ROOT, S.sorted[0], S.cnt[0], INF_LENS);
                inf_build_table(lane, S.lens + 288, 32, S.dist, INF_DIST_ROOT, S.sorted[1], S.cnt[1], INF_DISTS);
            } else {
                uint32_t hlit, hdist, hclen;
                if (!take(5, hlit) || !take(5, hdist) || !take(4, hclen)) INF_FAIL(RPCC_INFLATE_E_TRUNCATED);
                hlit += 257u, hdist += 1u, hclen += 4u;
                if (hlit > 286u || hdist > 30u) INF_FAIL(RPCC_INFLATE_E_TABLE);
                INF_SYNC();
                if (lane < 19) S.lens[lane] = 0;
                if (INF_WAVE < 19 && lane == 0)
                    for (int x = 1; x < 19; ++x) S.lens[x] = 0;
                INF_SYNC();
                for (uint32_t k = 0; k < hclen; ++k) {
                    uint32_t v;
                    if (!take(3, v)) INF_FAIL(RPCC_INFLATE_E_TRUNCATED);
                    if (lane == 0) S.lens[INF_CL_ORDER[k]] = (uint8_t)v;
                }
                INF_SYNC();
                if (inf_build_table(lane, S.lens, 19, S.cl, INF_CL_ROOT, nullptr, nullptr, INF_CODES)) INF_FAIL(RPCC_INFLATE_E_TABLE);
                const uint32_t total = hlit + hdist;
                uint32_t have = 0, prev = 0, len256 = 0;
                while (have < total) {
                    uint32_t s, v, r, x;
                    const int e = symbol(-1, S.cl, INF_CL_ROOT, s);
                    if (e) INF_FAIL(e);
                    if (s < 16u) {
                        v = s, r = 1u;
                    } else if (s == 16u) {
                        if (have == 0u) INF_FAIL(RPCC_INFLATE_E_TABLE);
                        if (!take(2, x)) INF_FAIL(RPCC_INFLATE_E_TRUNCATED);
                        v = prev, r = 3u + x;
                    } else if (s == 17u) {
                        if (!take(3, x)) INF_FAIL(RPCC_INFLATE_E_TRUNCATED);
                        v = 0u, r = 3u + x;
                    } else {
                        if (!take(7, x)) INF_FAIL(RPCC_INFLATE_E_TRUNCATED);
                        v = 0u, r = 11u + x;
                    }
                    if (have + r > total) INF_FAIL(RPCC_INFLATE_E_TABLE);
                    for (uint32_t y = lane; y < r; y += INF_WAVE) S.lens[have + y] = (uint8_t)v;
                    if (have <= 256u && 256u < have + r) len256 = v;
                    have += r;
                    prev = v;
                }
                if (len256 == 0u) INF_FAIL(RPCC_INFLATE_E_TABLE);
                INF_SYNC();
                if (inf_build_table(lane, S.lens, (int)hlit, S.lit, INF_LIT_ROOT, S.sorted[0], S.cnt[0], INF_LENS)) INF_FAIL(RPCC_INFLATE_E_TABLE);
                if (inf_build_table(lane, S.lens + hlit, (int)hdist, S.dist, INF_DIST_ROOT, S.sorted[1], S.cnt[1], INF_DISTS))
                    INF_FAIL(RPCC_INFLATE_E_TABLE);
            }
            for (;;) {
                if (op - flushed >= INF_FLUSH) {
                    INF_SYNC();
                    flush(INF_FLUSH);
                }
                uint32_t s, x;
                int e = symbol(0, S.lit, INF_LIT_ROOT, s);
                if (e) INF_FAIL(e);
                if (s < 256u) {
                    if (op >= cap) INF_FAIL(RPCC_INFLATE_E_OVERRUN);
                    if (lane == 0) S.ring[op & (INF_RING - 1)] = (uint8_t)s;
                    ++op;
                    continue;
                }
                if (s == 256u) break;
                if (s > 285u) INF_FAIL(RPCC_INFLATE_E_SYMBOL);
                if (!take(INF_LEN_EXTRA[s - 257u], x)) INF_FAIL(RPCC_INFLATE_E_TRUNCATED);
                const int64_t ml = (int64_t)(INF_LEN_BASE[s - 257u] + x);
                e = symbol(1, S.dist, INF_DIST_ROOT, s);
                if (e) INF_FAIL(e);
                if (s > 29u) INF_FAIL(RPCC_INFLATE_E_SYMBOL);
                if (!take(INF_DIST_EXTRA[s], x)) INF_FAIL(RPCC_INFLATE_E_TRUNCATED);
                const int64_t off = (int64_t)(INF_DIST_BASE[s] + x);
                if (off > op) INF_FAIL(RPCC_INFLATE_E_OFFSET);
                if (ml > cap - op) INF_FAIL(RPCC_INFLATE_E_OVERRUN);
                INF_SYNC();
                // out[op + k] = out[op - off + k].  P: the smallest multiple of off >= the wave.  k < P reads the history before op (periodic
                // in off); k >= P reads op + k - P, written by an earlier step.  Both lie within the last 32 KB.
                const int64_t P = off >= INF_WAVE ? off : off * ((INF_WAVE - 1 + off) / off);
                for (int64_t base = 0; base < ml; base += INF_WAVE) {
                    const int64_t k = base + lane;
                    uint8_t b = 0;
                    if (k < ml) {
                        const int64_t from = k < P ? op - off + (off > k ? k : (int64_t)((uint32_t)k % (uint32_t)off)) : op + k - P;
                        b = S.ring[from & (INF_RING - 1)];
                    }
                    INF_SYNC();   // at distances of 32768 - 63 and more, one lane's source is the ring slot another lane fills in this step
                    if (k < ml) S.ring[(op + k) & (INF_RING - 1)] = b;
                    INF_SYNC();
                }
                op += ml;
            }
        }
        if (final_) break;
    }
    INF_SYNC();
    while (op - flushed >= INF_FLUSH) flush(INF_FLUSH);
    if (op > flushed) flush(op - flushed);

    // ---- the trailer, then nothing or zero bytes
    to_byte();
    if (iend - ip < 8) INF_FAIL(RPCC_INFLATE_E_TRUNCATED);
    const uint32_t want_crc = get(ip) | get(ip + 1) << 8 | get(ip + 2) << 16 | get(ip + 3) << 24;
    const uint32_t want_size = get(ip + 4) | get(ip + 5) << 8 | get(ip + 6) << 16 | get(ip + 7) << 24;
    ip += 8;
    if (want_crc != (crc ^ 0xFFFFFFFFu)) INF_FAIL(RPCC_INFLATE_E_CRC);
    if (want_size != (uint32_t)op) INF_FAIL(RPCC_INFLATE_E_SIZE);
    bool nonzero = false;
    for (int64_t x = ip + lane; x < iend; x += INF_WAVE) nonzero = nonzero || in[x] != 0;
    if (INF_BALLOT(nonzero)) INF_FAIL(RPCC_INFLATE_E_TRAILING);
    INF_FAIL(RPCC_INFLATE_OK);
}

#endif  // RPCC_INFLATE_CORE_H
