// bunzip2_core.h -- the decoder of one bzip2 stream by one wavefront (tests/bunzip2_ref.py is its statement in
// Python).  bunzip2_kernels.hip includes it for gfx950; the including file defines how the wave is spoken to:
//   BZ_FN              function qualifiers (BZ_HD: those of the two layout functions, which the host calls too)
//   BZ_WAVE            lanes per wave (a power of two, at most 64)
//   BZ_SYNC()          barrier of the wave's LDS and work-slot traffic
//   BZ_UNI(x)          x, known to be equal in every lane, as a scalar (int)
//   BZ_BALLOT(p)       64-bit mask of the lanes where p holds
//   BZ_SHFL_XOR(v, m)  v of lane ^ m                  BZ_SHFL_UP(v, d)   v of lane - d (anything in the lanes below d)
//   BZ_READLANE(v, l)  v of lane l, l equal in every lane
//   BZ_LDS_ADD(p, v)   *p += v on a 32-bit word of the shared block, nothing returned
//   BZ_LDS_FETCH_ADD(p, v)  the same, returning the word's earlier value; atomic among the lanes
// With BZ_WAVE 1 and an empty BZ_SYNC the same text is an ordinary sequential bunzip2.
//
// Everything the symbol loop decides is equal in all lanes (bit buffer, positions, status).  The lanes part to build the tables, to hold
// the move-to-front list (four entries each), to sort the block's bytes into links, to walk the links as many sublists at once, and to
// expand the runs and fold the CRC.
#ifndef RPCC_BUNZIP2_CORE_H
#define RPCC_BUNZIP2_CORE_H

#include <stdint.h>

#define BZ_WIN 2048             // bytes of the input window
#define BZ_MAX_SELECTORS 18002
#define BZ_GROUP 50
#define BZ_MAX_LEN 20
#define BZ_RUN_LIMIT (2 * 1024 * 1024)
#define BZ_MAX_SPLIT 2048       // sublists of the walk: every stride-th link, and the origin
#define BZ_LEN_PER ((BZ_MAX_LEN + BZ_WAVE - 1) / BZ_WAVE)   // code lengths whose limit and base a lane holds
#define BZ_MTF_WORDS (64 / BZ_WAVE)   // 32-bit words of the move-to-front list in each lane: 256 entries over the wave

// The work slot of a stream whose blocks hold up to m bytes before the inverse RLE1: a 32-bit link for each position, then a byte.
// rpcc_bunzip2_stream_work_bytes() returns .bytes; the kernel carves the slot with the same call.
struct BzWorkLayout {
    int64_t tt, ll, bytes;      // offsets of uint32 tt[m] and uint8 ll[m]; the slot's size
};
BZ_HD BzWorkLayout bz_work_layout(int64_t m) {
    BzWorkLayout w;
    w.tt = 0;
    w.ll = 4 * m;
    w.bytes = 5 * m;
    return w;
}
// the longest block a slot of cap bytes holds
BZ_HD int64_t bz_work_block(int64_t cap) { return cap <= 0 ? 0 : cap / 5; }

struct BzShared {
    uint8_t win[BZ_WIN];                    // input bytes [wb, wb + BZ_WIN)
    uint8_t sel[BZ_MAX_SELECTORS + 2];      // the table of each group of 50 symbols
    int32_t limit[6][BZ_MAX_LEN + 2];       // libbz2's decode tables: the largest code of each length,
    int32_t base[6][BZ_MAX_LEN + 2];        // what to take from a code of that length to index perm,
    uint16_t perm[6][258];                  // the symbols by (length, symbol)
    uint8_t len[6][260];
    uint8_t minlen[8];
    uint32_t cftab[256];                    // bytes of each value in the block, then where the next one goes in sorted order
    uint32_t crc_tab[256];
    uint8_t seq[256];                       // the byte values in use, ascending
    uint32_t slen[BZ_MAX_SPLIT + 1];        // a sublist's length, then its offset in the block; scratch of the run expansion
    uint16_t ssucc[BZ_MAX_SPLIT + 2];       // the sublist that follows; BZ_ON_PATH once it has an offset
    uint32_t scal[4];                       // next sublist to hand out; the cycle's length
};
#define BZ_ON_PATH 0x8000u
static_assert(BZ_WAVE * 6 * 4 <= (BZ_MAX_SPLIT + 1) * 4, "the run expansion keeps six words per lane in slen");

// a * b in GF(2)[x] modulo bzip2's CRC polynomial, bit 31 = x^31
BZ_FN uint32_t bz_gf_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 31; i >= 0; --i) {
        p = (p << 1) ^ (0x04C11DB7u & (0u - (p >> 31)));
        p ^= b & (0u - ((a >> i) & 1u));
    }
    return p;
}

// x^(8 * bytes): what a CRC register is multiplied by when `bytes` more bytes follow
BZ_FN uint32_t bz_gf_pow8(uint32_t bytes) {
    uint32_t p = 1u, base = 0x100u;
    for (; bytes; bytes >>= 1) {
        if (bytes & 1u) p = bz_gf_mul(p, base);
        base = bz_gf_mul(base, base);
    }
    return p;
}

// libbz2's BZ2_hbCreateDecodeTables for table t over S.len[t][0 .. alpha): limit, base, perm and minlen.  Every lane takes symbols lane,
// lane + BZ_WAVE, ...; a symbol's rank among those of its length comes from ballots.  The lengths are 1 .. 20 (checked while they are read).
BZ_FN void bz_build_table(BzShared &S, const int lane, const int t, const int alpha) {
    int cnt[BZ_MAX_LEN + 1], offs[BZ_MAX_LEN + 1];
#pragma unroll
    for (int b = 0; b <= BZ_MAX_LEN; ++b) cnt[b] = 0;
    for (int s0 = 0; s0 < alpha; s0 += BZ_WAVE) {
        const int s = s0 + lane, L = s < alpha ? S.len[t][s] : 0;
#pragma unroll
        for (int b = 1; b <= BZ_MAX_LEN; ++b) cnt[b] += __builtin_popcountll(BZ_BALLOT(L == b));
    }
    int lo = 0, hi = 0, o = 0;
#pragma unroll
    for (int b = 1; b <= BZ_MAX_LEN; ++b) {
        if (cnt[b]) {
            if (!lo) lo = b;
            hi = b;
        }
        offs[b] = o;
        o += cnt[b];
    }
    if (lane == 0) {
        // limit[i] = vec - 1 with vec the codes of length i and less, doubled from length to length; base[i] turns a code into its rank
        int vec = 0, prev_limit = 0;
        for (int b = 0; b <= BZ_MAX_LEN + 1; ++b) {
            int lim = 0, bas = 0;
            if (b >= lo && b <= hi) {
                vec += cnt[b];
                lim = vec - 1;
                bas = b == lo ? 0 : ((prev_limit + 1) << 1) - offs[b];
                vec <<= 1;
                prev_limit = lim;
            }
            S.limit[t][b] = lim;
            S.base[t][b] = bas;
        }
        S.minlen[t] = (uint8_t)lo;
    }
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int s0 = 0; s0 < alpha; s0 += BZ_WAVE) {
        const int s = s0 + lane, L = s < alpha ? S.len[t][s] : 0;
        int idx = 0;
#pragma unroll
        for (int b = 1; b <= BZ_MAX_LEN; ++b) {
            const unsigned long long m = BZ_BALLOT(L == b);
            if (L == b) idx = offs[b] + __builtin_popcountll(m & below);
            offs[b] += __builtin_popcountll(m);
        }
        if (L) S.perm[t][idx] = (uint16_t)s;
    }
    BZ_SYNC();
}

#define BZ_FAIL(code)                   \
    do {                                \
        op_out = op;                    \
        used_out = ip - (bc >> 3);      \
        return (code);                  \
    } while (0)

// One stream: in[0, iend) -> out[0, cap), through the work slot `work` of work_cap bytes (4-byte aligned).
// -> status; op_out = bytes produced (with E_OVERRUN: the size the stream decodes to); used_out = input bytes read.
BZ_FN int bunzip2_stream(BzShared &S, const int lane, const uint8_t *__restrict__ in, const int64_t iend, uint8_t *__restrict__ out,
                         const int64_t cap, uint8_t *work, const int64_t work_cap, int64_t &op_out, int64_t &used_out) {
    int64_t op = 0;                  // bytes the blocks so far decode to
    int64_t ip = 0;                  // the next input byte that enters the bit buffer
    uint64_t bb = 0;                 // bc valid bits at the low end, most significant first; stale bits above them
    int bc = 0;
    const int64_t slot_block = ((uintptr_t)work & 3u) ? 0 : bz_work_block(work_cap);
    const BzWorkLayout lay = bz_work_layout(slot_block);
    uint32_t *tt = (uint32_t *)(work + lay.tt);
    uint8_t *ll = work + lay.ll;
    for (int i = lane; i < 256; i += BZ_WAVE) {
        uint32_t r = (uint32_t)i << 24;
        for (int k = 0; k < 8; ++k) r = (r << 1) ^ (0x04C11DB7u & (0u - (r >> 31)));
        S.crc_tab[i] = r;
    }
    int64_t wb = -BZ_WIN;            // window base: empty
    auto get = [&](int64_t at) -> uint32_t {   // one input byte at 0 <= at < iend, through the window (every lane asks for the same one)
        if (at < wb || at >= wb + BZ_WIN) {
            BZ_SYNC();
            wb = at;
            for (int64_t x = lane; x < BZ_WIN && wb + x < iend; x += BZ_WAVE) S.win[x] = in[wb + x];
            BZ_SYNC();
        }
        return (uint32_t)BZ_UNI(S.win[at - wb]);
    };
    auto refill = [&]() {            // brings bc to 56 or more, or to all that is left
        if (bc < 56 && ip >= wb && ip + 8 <= wb + BZ_WIN && ip + 8 <= iend) {   // eight window bytes in one round trip, the whole ones kept
            const uint8_t *w = S.win + (ip - wb);
            const uint32_t hi = (uint32_t)w[0] << 24 | (uint32_t)w[1] << 16 | (uint32_t)w[2] << 8 | (uint32_t)w[3];
            const uint32_t lo = (uint32_t)w[4] << 24 | (uint32_t)w[5] << 16 | (uint32_t)w[6] << 8 | (uint32_t)w[7];
            const int nb = (63 - bc) >> 3;   // 1 .. 7 bytes fit
            const uint64_t v = (uint64_t)(uint32_t)BZ_UNI(hi) << 32 | (uint32_t)BZ_UNI(lo);
            bb = (bb << (8 * nb)) | (v >> (64 - 8 * nb));
            bc += 8 * nb;
            ip += nb;
            return;
        }
        while (bc <= 56 && ip < iend) {
            bb = (bb << 8) | get(ip);
            bc += 8;
            ++ip;
        }
    };
    auto take = [&](int n, uint32_t &v) -> bool {   // n <= 32 bits; false: the input ends first, and nothing is taken
        if (bc < n) {
            refill();
            if (bc < n) return false;
        }
        v = (uint32_t)((bb >> (bc - n)) & ((1ull << n) - 1ull));
        bc -= n;
        return true;
    };
    uint32_t v, v2;

    // ---- the stream's header
    for (int k = 0; k < 3; ++k) {
        if (!take(8, v)) BZ_FAIL(RPCC_BUNZIP2_E_TRUNCATED);
        if (v != (k == 0 ? 0x42u : k == 1 ? 0x5Au : 0x68u)) BZ_FAIL(RPCC_BUNZIP2_E_HEADER);
    }
    if (!take(8, v)) BZ_FAIL(RPCC_BUNZIP2_E_TRUNCATED);
    if (v < 0x31u || v > 0x39u) BZ_FAIL(RPCC_BUNZIP2_E_HEADER);
    const int64_t block_max = 100000 * (int64_t)(v - 0x30u);
    uint32_t combined = 0;

    for (;;) {
        // ---- block header
        if (!take(24, v) || !take(24, v2)) BZ_FAIL(RPCC_BUNZIP2_E_TRUNCATED);
        if (v == 0x177245u && v2 == 0x385090u) break;
        if (v != 0x314159u || v2 != 0x265359u) BZ_FAIL(RPCC_BUNZIP2_E_MAGIC);
        uint32_t block_crc, orig;
        if (!take(32, block_crc) || !take(1, v)) BZ_FAIL(RPCC_BUNZIP2_E_TRUNCATED);
        if (v) BZ_FAIL(RPCC_BUNZIP2_E_RANDOMISED);
        if (!take(24, orig)) BZ_FAIL(RPCC_BUNZIP2_E_TRUNCATED);
        if ((int64_t)orig > 10 + block_max) BZ_FAIL(RPCC_BUNZIP2_E_ORIGPTR);
        uint32_t used16;
        if (!take(16, used16)) BZ_FAIL(RPCC_BUNZIP2_E_TRUNCATED);
        BZ_SYNC();                   // the previous block is done with the shared tables
        int in_use = 0;
        for (int i = 0; i < 16; ++i) {
            if (!((used16 >> (15 - i)) & 1u)) continue;
            if (!take(16, v)) BZ_FAIL(RPCC_BUNZIP2_E_TRUNCATED);
            for (int k = 0; k < 16; ++k) {
                if ((v >> (15 - k)) & 1u) {
                    if (lane == 0) S.seq[in_use] = (uint8_t)(16 * i + k);
                    ++in_use;
                }
            }
        }
        if (in_use == 0) BZ_FAIL(RPCC_BUNZIP2_E_TABLE);
        const int alpha = in_use + 2, eob = in_use + 1;
        uint32_t ngroups, nsel_read;
        if (!take(3, ngroups)) BZ_FAIL(RPCC_BUNZIP2_E_TRUNCATED);
        if (ngroups < 2u || ngroups > 6u) BZ_FAIL(RPCC_BUNZIP2_E_TABLE);
        if (!take(15, nsel_read)) BZ_FAIL(RPCC_BUNZIP2_E_TRUNCATED);
        if (nsel_read < 1u) BZ_FAIL(RPCC_BUNZIP2_E_TABLE);
        // selectors: unary indices into a move-to-front list of the tables, kept as six nibbles; those past 18002 are read and dropped
        uint32_t order = 0x543210u;
        for (uint32_t i = 0; i < nsel_read; ++i) {
            uint32_t j = 0;
            for (;;) {
                if (!take(1, v)) BZ_FAIL(RPCC_BUNZIP2_E_TRUNCATED);
                if (!v) break;
                if (++j >= ngroups) BZ_FAIL(RPCC_BUNZIP2_E_TABLE);
            }
            if (i < BZ_MAX_SELECTORS) {
                const uint32_t t = (order >> (4 * j)) & 15u, low = order & ((1u << (4 * j)) - 1u);
                order = (order & ~((1u << (4 * j + 4)) - 1u)) | low << 4 | t;
                if (lane == 0) S.sel[i] = (uint8_t)t;
            }
        }
        const int nsel = (int)(nsel_read < BZ_MAX_SELECTORS ? nsel_read : BZ_MAX_SELECTORS);
        for (uint32_t t = 0; t < ngroups; ++t) {
            uint32_t curr;
            if (!take(5, curr)) BZ_FAIL(RPCC_BUNZIP2_E_TRUNCATED);
            for (int i = 0; i < alpha; ++i) {
                for (;;) {
                    if (curr < 1u || curr > BZ_MAX_LEN) BZ_FAIL(RPCC_BUNZIP2_E_TABLE);
                    if (!take(1, v)) BZ_FAIL(RPCC_BUNZIP2_E_TRUNCATED);
                    if (!v) break;
                    if (!take(1, v)) BZ_FAIL(RPCC_BUNZIP2_E_TRUNCATED);
                    curr += v ? 0xFFFFFFFFu : 1u;
                }
                if (lane == 0) S.len[t][i] = (uint8_t)curr;
            }
        }
        for (int x = lane; x < 256; x += BZ_WAVE) S.cftab[x] = 0;
        BZ_SYNC();
        for (uint32_t t = 0; t < ngroups; ++t) bz_build_table(S, lane, (int)t, alpha);

        // ---- symbols.  The move-to-front list holds byte values: entry p in byte p & 3 of word p >> 2, word g in lane g / BZ_MTF_WORDS.
        uint32_t mtf[BZ_MTF_WORDS];
#pragma unroll
        for (int j = 0; j < BZ_MTF_WORDS; ++j) {
            const int p = 4 * (lane * BZ_MTF_WORDS + j);
            uint32_t w = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) w |= (uint32_t)(p + k < in_use ? S.seq[p + k] : 0) << (8 * k);
            mtf[j] = w;
        }
        uint32_t front4 = (uint32_t)BZ_READLANE(mtf[0], 0);   // the list's first four entries, equal in all lanes: most moves end here
        int group_no = -1, group_pos = 0, gsel = 0, gmin = 0;
        // One symbol by libbz2's rule: gmin bits, then one more while the code exceeds limit[length]; 20 bits at most -> 0 or a status.
        // The lengths are dealt over the lanes -- lane l holds limit and base of the lengths l + 1, l + 1 + BZ_WAVE, ... of the group's
        // table -- and every lane tests its length against the next 20 bits: the shortest length that passes is the rule's answer.
        int lim[BZ_LEN_PER], bas[BZ_LEN_PER];
        auto symbol = [&](uint32_t &sym) -> int {
            if (group_pos == 0) {
                if (++group_no >= nsel) return RPCC_BUNZIP2_E_SYMBOL;
                group_pos = BZ_GROUP;
                gsel = BZ_UNI(S.sel[group_no]);
                gmin = BZ_UNI(S.minlen[gsel]);
#pragma unroll
                for (int j = 0; j < BZ_LEN_PER; ++j) {
                    const int k = 1 + lane + j * BZ_WAVE;
                    lim[j] = k <= BZ_MAX_LEN ? S.limit[gsel][k] : -1;
                    bas[j] = k <= BZ_MAX_LEN ? S.base[gsel][k] : 0;
                }
            }
            --group_pos;
            if (bc < BZ_MAX_LEN + 1) refill();
            if (bc < gmin) return RPCC_BUNZIP2_E_TRUNCATED;
            const uint32_t peek = (uint32_t)(bc >= BZ_MAX_LEN ? bb >> (bc - BZ_MAX_LEN) : bb << (BZ_MAX_LEN - bc)) & ((1u << BZ_MAX_LEN) - 1u);
            const int have = bc < BZ_MAX_LEN ? bc : BZ_MAX_LEN;
#pragma unroll
            for (int j = 0; j < BZ_LEN_PER; ++j) {
                const int k = 1 + lane + j * BZ_WAVE;
                const int zvec = k <= BZ_MAX_LEN ? (int)(peek >> (BZ_MAX_LEN - k)) : 0;
                const unsigned long long hit = BZ_BALLOT(k >= gmin && k <= have && zvec <= lim[j]);
                if (hit) {
                    const int first = __builtin_ctzll(hit);
                    const int idx = BZ_READLANE(zvec - bas[j], first);
                    bc -= 1 + first + j * BZ_WAVE;
                    if (idx < 0 || idx >= alpha) return RPCC_BUNZIP2_E_SYMBOL;
                    sym = (uint32_t)BZ_UNI(S.perm[gsel][idx]);
                    return 0;
                }
            }
            if (bc <= BZ_MAX_LEN) {  // the next bit is past the end: the bits so far count as read
                bc = 0;
                return RPCC_BUNZIP2_E_TRUNCATED;
            }
            bc -= BZ_MAX_LEN + 1;    // libbz2 reads the 21st bit before it gives up
            return RPCC_BUNZIP2_E_SYMBOL;
        };
        int64_t nblock = 0;
        uint32_t acc = 0;            // the block's bytes gather here, one per lane, and leave BZ_WAVE at a time
        auto emit = [&](uint32_t uc, int64_t n) {   // n copies of uc at ll[nblock ..); room was checked
            while (n > 0) {
                const int at = (int)(nblock & (BZ_WAVE - 1));
                const int64_t piece = n < BZ_WAVE - at ? n : BZ_WAVE - at;
                if (lane >= at && lane < at + piece) acc = uc;
                nblock += piece;
                n -= piece;
                if (at + piece == BZ_WAVE) ll[nblock - BZ_WAVE + lane] = (uint8_t)acc;
            }
        };
        uint32_t sym;
        int e = symbol(sym);
        if (e) BZ_FAIL(e);
        while ((int)sym != eob) {
            if (sym <= 1u) {
                int64_t es = -1, n = 1;
                do {
                    if (n >= BZ_RUN_LIMIT) BZ_FAIL(RPCC_BUNZIP2_E_SYMBOL);
                    es += n << sym;
                    n <<= 1;
                    e = symbol(sym);
                    if (e) BZ_FAIL(e);
                } while (sym <= 1u);
                ++es;
                if (nblock + es > block_max) BZ_FAIL(RPCC_BUNZIP2_E_SYMBOL);
                if (nblock + es > slot_block) BZ_FAIL(RPCC_BUNZIP2_E_WORK);
                emit(front4 & 255u, es);
                continue;
            }
            if (nblock + 1 > block_max) BZ_FAIL(RPCC_BUNZIP2_E_SYMBOL);
            if (nblock + 1 > slot_block) BZ_FAIL(RPCC_BUNZIP2_E_WORK);
            // move entry nn to the front: the entries before it shift up by one, a byte from word to word and from lane to lane
            const int nn = (int)sym - 1, gw = nn >> 2, k = nn & 3;
            const uint32_t keep = k == 3 ? 0u : 0xFFFFFFFFu << (8 * (k + 1));   // the bytes of word gw behind entry nn
            uint32_t front;
            if (gw == 0) {
                front = (front4 >> (8 * k)) & 255u;
                front4 = ((front4 << 8 | front) & ~keep) | (front4 & keep);
            } else {
                if (lane == 0) mtf[0] = front4;
                front = ((uint32_t)BZ_READLANE(mtf[gw % BZ_MTF_WORDS], gw / BZ_MTF_WORDS) >> (8 * k)) & 255u;
                const uint32_t carry_in = (uint32_t)BZ_SHFL_UP(mtf[BZ_MTF_WORDS - 1], 1) >> 24;
#pragma unroll
                for (int j = BZ_MTF_WORDS - 1; j >= 0; --j) {
                    const int g = lane * BZ_MTF_WORDS + j;
                    const uint32_t from = g == 0 ? front : j > 0 ? mtf[j - 1] >> 24 : carry_in;
                    const uint32_t moved = mtf[j] << 8 | from;
                    if (g < gw) mtf[j] = moved;
                    if (g == gw) mtf[j] = (moved & ~keep) | (mtf[j] & keep);
                }
                front4 = (uint32_t)BZ_READLANE(mtf[0], 0);
            }
            emit(front, 1);
            e = symbol(sym);
            if (e) BZ_FAIL(e);
        }
        if (nblock & (BZ_WAVE - 1)) {
            const int64_t b0 = nblock & ~(int64_t)(BZ_WAVE - 1);
            if (b0 + lane < nblock) ll[b0 + lane] = (uint8_t)acc;
        }
        if ((int64_t)orig >= nblock) BZ_FAIL(RPCC_BUNZIP2_E_ORIGPTR);
        BZ_SYNC();

        // ---- links: the stable counting sort of the block's bytes.  tt[j] = i << 8 | byte for the j-th byte in sorted order, which stands
        // at position i: the text is byte(tt[p]), p = tt[p] >> 8, from p = orig.
        {
            // cftab: the bytes of each value, counted by all lanes, -> where each value's first byte goes (an exclusive scan: 256 / BZ_WAVE
            // entries per lane, then over the lanes)
            for (int64_t i = lane; i < nblock; i += BZ_WAVE) BZ_LDS_ADD(&S.cftab[ll[i]], 1u);
            BZ_SYNC();
            const int per = 256 / BZ_WAVE;
            uint32_t sum = 0;
            for (int x = 0; x < per; ++x) sum += S.cftab[lane * per + x];
            uint32_t incl = sum;
            for (int d = 1; d < BZ_WAVE; d <<= 1) {
                const uint32_t up = (uint32_t)BZ_SHFL_UP(incl, d);
                if (lane >= d) incl += up;
            }
            uint32_t run = incl - sum;
            BZ_SYNC();
            for (int x = 0; x < per; ++x) {
                const uint32_t c = S.cftab[lane * per + x];
                S.cftab[lane * per + x] = run;
                run += c;
            }
            BZ_SYNC();
            const unsigned long long below = (1ull << lane) - 1ull;
            for (int64_t i0 = 0; i0 < nblock; i0 += BZ_WAVE) {
                const int64_t i = i0 + lane;
                const bool live = i < nblock;
                const uint32_t uc = live ? ll[i] : 0u;
                unsigned long long peers = BZ_BALLOT(live);   // the lanes with the same byte
#pragma unroll
                for (int b = 0; b < 8; ++b) {
                    const unsigned long long m = BZ_BALLOT((uc >> b) & 1u);
                    peers &= ((uc >> b) & 1u) ? m : ~m;
                }
                uint32_t at = 0;
                bool moves = false;          // the last of the byte's lanes moves its place on
                if (live) {
                    const int rank = __builtin_popcountll(peers & below), all = __builtin_popcountll(peers);
                    at = S.cftab[uc] + (uint32_t)rank;
                    moves = rank == all - 1;
                }
                BZ_SYNC();                   // every lane of the byte has read its place before one of them writes it
                if (moves) S.cftab[uc] = at + 1u;
                if (live) tt[at] = (uint32_t)i << 8 | uc;
                BZ_SYNC();
            }
        }

        // ---- the walk, as sublists: a splitter at every stride-th link and at the origin.  Pass 1: each lane walks from a splitter to the
        // next one and notes length and successor.  Then the splitters are followed from the origin and given their offsets in the text,
        // until the block is covered or the cycle closes.  Pass 2: each lane walks its sublists again and stores the bytes.  tt is a
        // permutation whatever the block holds, so every walk ends at a splitter after at most nblock steps.
        {
            int shift = 0;
            while (((nblock - 1) >> shift) + 1 > BZ_MAX_SPLIT) ++shift;
#ifdef BZ_SERIAL_WALK            // developer builds only (tools_dev/bunzip2_time.py): link 0 and the origin are the only splitters
            shift = 31;
#endif
            const uint32_t mask = (1u << shift) - 1u;
            const int ngrid = (int)(((nblock - 1) >> shift) + 1);
            const bool extra = (orig & mask) != 0;           // the origin is a splitter of its own
            const int nsplit = ngrid + (extra ? 1 : 0);
            auto is_split = [&](uint32_t p) { return (p & mask) == 0 || p == orig; };
            auto id_of = [&](uint32_t p) { return extra && p == orig ? ngrid : (int)(p >> shift); };
            auto start_of = [&](int id) { return id == ngrid ? orig : (uint32_t)id << shift; };
            uint8_t *pre = ll;                  // the text overwrites the block's bytes, which the links no longer need
            for (int pass = 0; pass < 2; ++pass) {
                if (lane == 0) S.scal[0] = 0;
                BZ_SYNC();
                int id = -1;
                uint32_t p = 0, n = 0, at = 0;
                bool done = false;
                while (BZ_BALLOT(!done)) {
                    if (!done && id < 0) {
                        for (;;) {   // the next sublist; in pass 2 one that lies on the path
                            id = (int)BZ_LDS_FETCH_ADD(&S.scal[0], 1u);
                            if (id >= nsplit) {
                                done = true;
                                break;
                            }
                            if (pass == 0 || (S.ssucc[id] & BZ_ON_PATH)) break;
                        }
                        if (!done) {
                            p = start_of(id);
                            n = 0;
                            at = pass ? S.slen[id] : 0;
                        }
                    }
                    if (!done) {
                        const uint32_t link = tt[p];
                        if (pass) pre[at + n] = (uint8_t)link;
                        ++n;
                        p = link >> 8;
                        if (is_split(p)) {
                            if (pass == 0) {
                                S.slen[id] = n;
                                S.ssucc[id] = (uint16_t)id_of(p);
                            }
                            id = -1;
                        }
                    }
                }
                BZ_SYNC();
                if (pass == 0) {
                    if (lane == 0) {
                        const int first = id_of(orig);
                        int cur = first;
                        uint32_t off = 0;
                        do {
                            const uint32_t len = S.slen[cur];
                            const int nxt = S.ssucc[cur];
                            S.slen[cur] = off;
                            S.ssucc[cur] = (uint16_t)(nxt | BZ_ON_PATH);
                            off += len;
                            cur = nxt;
                        } while (off < (uint32_t)nblock && cur != first);
                        S.scal[1] = off;
                    }
                    BZ_SYNC();
                }
            }
            // a cycle shorter than the block: the text repeats with the cycle's length
            const int64_t period = (int64_t)(uint32_t)BZ_UNI(S.scal[1]);
            for (int64_t x = period + lane; x < nblock; x += BZ_WAVE) pre[x] = pre[x % period];
            BZ_SYNC();

            // ---- inverse RLE1, CRC and stores.  Lane l takes the text's bytes [l * chunk, (l + 1) * chunk).  The state at a byte is how many
            // equal bytes end just before it: 0 after a count byte or at the block's start, 1 .. 3, and 4 when this byte is the count.  Each
            // lane follows all five states through its chunk (pass A: where they end, how many bytes they give); the chain from lane to lane
            // picks the true one; then the lane expands its chunk from it (pass B).
            const int64_t chunk = (nblock + BZ_WAVE - 1) / BZ_WAVE;
            const int64_t a = lane * chunk < nblock ? lane * chunk : nblock, b = a + chunk < nblock ? a + chunk : nblock;
            uint32_t *__restrict__ scratch = S.slen;
            {
                uint32_t st[5], len[5];
#pragma unroll
                for (int s = 0; s < 5; ++s) st[s] = (uint32_t)s, len[s] = 0;
                uint32_t prev = a > 0 ? pre[a - 1] : 0u;
                for (int64_t x = a; x < b; ++x) {
                    const uint32_t by = pre[x];
#pragma unroll
                    for (int s = 0; s < 5; ++s) {
                        if (st[s] == 4u) {
                            len[s] += by;
                            st[s] = 0;
                        } else {
                            st[s] = st[s] && by == prev ? st[s] + 1u : 1u;
                            ++len[s];
                        }
                    }
                    prev = by;
                }
                uint32_t map = 0;
#pragma unroll
                for (int s = 0; s < 5; ++s) {
                    map |= st[s] << (3 * s);
                    scratch[6 * lane + 1 + s] = len[s];
                }
                scratch[6 * lane] = map;
            }
            BZ_SYNC();
            uint32_t my_state = 0, state = 0;
            int64_t my_off = 0, total = 0;
            for (int l = 0; l < BZ_WAVE; ++l) {
                if (l == lane) {
                    my_state = state;
                    my_off = total;
                }
                total += scratch[6 * l + 1 + state];
                state = (scratch[6 * l] >> (3 * state)) & 7u;
            }
            BZ_SYNC();
            if (state == 4u) BZ_FAIL(RPCC_BUNZIP2_E_RLE);    // four equal bytes end the block: libbz2 reads a count from beyond it and refuses
            uint32_t reg = lane == 0 ? 0xFFFFFFFFu : 0u;
            int64_t o = op + my_off;
            {
                uint32_t c = my_state, prev = a > 0 ? pre[a - 1] : 0u;
                for (int64_t x = a; x < b; ++x) {
                    const uint32_t by = pre[x];
                    if (c == 4u) {
                        for (uint32_t r = 0; r < by; ++r) {
                            if (o < cap) out[o] = (uint8_t)prev;
                            ++o;
                            reg = (reg << 8) ^ S.crc_tab[(reg >> 24) ^ prev];
                        }
                        c = 0;
                        continue;            // prev stays: state 0 never compares with it
                    }
                    c = c && by == prev ? c + 1u : 1u;
                    if (o < cap) out[o] = (uint8_t)by;
                    ++o;
                    reg = (reg << 8) ^ S.crc_tab[(reg >> 24) ^ by];
                    prev = by;
                }
            }
            // reg(A ++ B) = reg(A) * x^(8 |B|) + reg0(B): every lane's register times x^(8 * the bytes behind its chunk), summed
            reg = bz_gf_mul(reg, bz_gf_pow8((uint32_t)(op + total - o)));
            for (int k = 1; k < BZ_WAVE; k <<= 1) reg ^= (uint32_t)BZ_SHFL_XOR(reg, k);
            op += total;
            const uint32_t have = ~reg;
            if (have != block_crc) BZ_FAIL(RPCC_BUNZIP2_E_CRC);
            combined = (combined << 1 | combined >> 31) ^ have;
        }
    }

    // ---- the end of the stream: the combined CRC, padding to a byte, then nothing
    if (!take(32, v)) BZ_FAIL(RPCC_BUNZIP2_E_TRUNCATED);
    bc -= bc & 7;
    if (v != combined) BZ_FAIL(RPCC_BUNZIP2_E_CRC);
    if (ip - (bc >> 3) < iend) BZ_FAIL(RPCC_BUNZIP2_E_TRAILING);
    BZ_FAIL(op > cap ? RPCC_BUNZIP2_E_OVERRUN : RPCC_BUNZIP2_OK);
}

#endif  // RPCC_BUNZIP2_CORE_H
