// bzip2_core.h -- the encoder of one bzip2 stream by one workgroup (tests/bzip2_ref.py is its statement in Python).
// bzip2_kernels.hip includes it for gfx950; the including file defines how the workgroup is spoken to:
//   BZE_FN             function qualifiers (BZE_HD: those of the layout and bound functions, which the host calls too)
//   BZE_T              threads of the workgroup          BZE_WAVE   lanes per wave (a power of two, at most 64, dividing BZE_T)
//   BZE_SYNC()         barrier of the workgroup's LDS and work-slot traffic
//   BZE_BALLOT(p)      64-bit mask of the wave's lanes where p holds
//   BZE_SHFL_UP(v, d)  v of lane - d (anything in the lanes below d)
//   BZE_LDS_ADD(p, v)  *p += v        BZE_LDS_OR(p, v)  *p |= v        BZE_LDS_XOR(p, v)  *p ^= v   on a 32-bit word of the shared block
// With BZE_T 1, BZE_WAVE 1 and an empty BZE_SYNC the same text is an ordinary sequential encoder (tests/bzip2_host_main.cpp).
//
// No stage waits on another workgroup and every loop is bounded by a count read from the code: the block's bytes, its chunks, 256 bins,
// BZE_MAX_ROUNDS doubling rounds.  Order never comes from an atomic: a key's place in a radix pass is its bin's start, the counts of the
// waves before it (LDS words each wave writes alone) and its rank among the wave's equal keys (ballots).
#ifndef RPCC_BZIP2_CORE_H
#define RPCC_BZIP2_CORE_H

#include <stdint.h>

#define BZE_GROUP 50
#define BZE_MAX_LEN 17              // bits of the longest code
#define BZE_PASSES 4                // refinement passes of the tables
#define BZE_MAX_ROUNDS 21           // doubling rounds: ceil(log2(900000)) + 1
#define BZE_MTF_CHUNK 256           // the fewest bytes of a move-to-front chunk
#define BZE_EMIT_ITEMS 4            // symbols per thread and step of the emit stage
#define BZE_NW (BZE_T / BZE_WAVE)
#define BZE_MAX_INPUT 0x7E000000
#define BZE_STAGE_WORDS (BZE_T * BZE_EMIT_ITEMS * BZE_MAX_LEN / 32 + 3)

BZE_HD int64_t bze_block_limit(int level) { return 100000 * (int64_t)level - 19; }
// the most RLE1 bytes a stream of n bytes keeps in one block of this level
BZE_HD int64_t bze_block_cap(int64_t n, int level) {
    const int64_t m = n + n / 4, lim = bze_block_limit(level);
    return m < lim ? m : lim;
}

// The worst case of the specification, in bytes (bzip2_ref.bound): m = n + n / 4 RLE1 bytes in nb blocks, each cut at most 4 bytes below
// the limit; 17 bits a symbol, one symbol a byte and the end symbol; 6 bits a group of 50; per block 54 bytes of header and maps and six
// tables of 5 + 258 * 33 bits; 4 + 10 bytes around the blocks.
BZE_HD int64_t bze_bound(int64_t n, int level) {
    if (n < 0 || n > BZE_MAX_INPUT || level < 1 || level > 9) return 0;
    const int64_t m = n + n / 4, per = bze_block_limit(level) - 4;
    int64_t nb = (m + per - 1) / per;
    if (nb < 1) nb = 1;
    const int64_t sym_bits = 17 * (m + nb), sel_bits = 6 * ((m + nb) / BZE_GROUP + nb);
    return 14 + nb * (19 + 32 + 3 + 6 * 1066) + (sym_bits + sel_bits + 7) / 8;
}

// The work slot of a stream whose block holds up to m RLE1 bytes.  rpcc_bzip2_workspace_bytes sums .bytes; the kernel carves with the same call.
struct BzeLayout {
    int64_t sa, sa2, rank, rank2;   // uint32 [m16] each: the rotations in order and its other copy, each rotation's rank and its other copy
    int64_t rle, last;              // uint8 [m16]: the block after RLE1; the last column, then the move-to-front ranks
    int64_t sym;                    // uint16 [m16 + 16]: the symbols after RLE2
    int64_t sel;                    // uint8: the table of each group
    int64_t lists, states;          // uint8 [chunks][256]: each chunk's recency list; the list a chunk starts from
    int64_t bytes;
};
BZE_HD BzeLayout bze_layout(int64_t m) {
    BzeLayout w;
    const int64_t m16 = m < 16 ? 16 : (m + 15) & ~(int64_t)15, chunks = m16 / BZE_MTF_CHUNK + 1;
    w.sa = 0;
    w.sa2 = 4 * m16;
    w.rank = 8 * m16;
    w.rank2 = 12 * m16;
    w.rle = 16 * m16;
    w.last = 17 * m16;
    w.sym = 18 * m16;
    w.sel = w.sym + 2 * m16 + 32;
    w.lists = w.sel + ((m16 / BZE_GROUP + 2 + 15) & ~(int64_t)15);
    w.states = w.lists + 256 * chunks;
    w.bytes = w.states + 256 * chunks;
    return w;
}
// an upper bound of the slots of nstreams streams of total_len bytes in all: .bytes <= 23 * m16 + 576 and m16 <= n + n / 4 + 16
BZE_HD int64_t bze_slots_bytes(int64_t nstreams, int64_t total_len) { return 23 * (total_len + total_len / 4) + 944 * nstreams; }

struct BzeShared {
    uint32_t crc_tab[256];
    uint32_t hist[256], base[256];          // keys of each digit; where the next key of each digit goes
    uint32_t wcnt[BZE_NW][256];             // keys of each digit in each wave of the tile
    uint32_t wsum[BZE_NW + 1];
    uint32_t scal[16];
    uint32_t tail[BZE_T];                   // per chunk: the equal bytes at its end; its list's length; the zero ranks at its end
    uint32_t freq[258];
    uint32_t rfreq[6][258];
    uint32_t code[6][258];                  // length << 24 | code
    uint32_t weight[6][2 * 258];            // leaves in sorted order, then internal nodes in creation order
    uint16_t parent[6][2 * 258], depth[6][2 * 258], order[6][258];
    uint32_t num[6][BZE_MAX_LEN + 2];
    uint32_t stage[BZE_STAGE_WORDS];        // a step's bits, most significant first, from the carried partial byte on
    uint8_t len[6][260];
    uint8_t seq[256], unseq[256];           // the byte values in use, ascending; a value's place among them
};
enum { BZE_S_CRC = 0, BZE_S_NFLAG, BZE_S_ORIG, BZE_S_NUSED, BZE_S_POS, BZE_S_CB, BZE_S_CARRY };

// a * b in GF(2)[x] modulo bzip2's CRC polynomial, bit 31 = x^31
BZE_FN uint32_t bze_gf_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 31; i >= 0; --i) {
        p = (p << 1) ^ (0x04C11DB7u & (0u - (p >> 31)));
        p ^= b & (0u - ((a >> i) & 1u));
    }
    return p;
}
// x^(8 * bytes): what a CRC register is multiplied by when `bytes` more bytes follow
BZE_FN uint32_t bze_gf_pow8(uint32_t bytes) {
    uint32_t p = 1u, base = 0x100u;
    for (; bytes; bytes >>= 1) {
        if (bytes & 1u) p = bze_gf_mul(p, base);
        base = bze_gf_mul(base, base);
    }
    return p;
}

// Exclusive sum of v over the workgroup's threads; total = the sum.  Ends with a barrier.
BZE_FN uint32_t bze_scan_add(BzeShared &S, const int tid, const uint32_t v, uint32_t &total) {
    const int lane = tid % BZE_WAVE, wave = tid / BZE_WAVE;
    uint32_t incl = v;
    for (int d = 1; d < BZE_WAVE; d <<= 1) {
        const uint32_t up = (uint32_t)BZE_SHFL_UP(incl, d);
        if (lane >= d) incl += up;
    }
    if (lane == BZE_WAVE - 1) S.wsum[wave] = incl;
    BZE_SYNC();
    uint32_t off = 0, tot = 0;
    for (int w = 0; w < BZE_NW; ++w) {
        const uint32_t x = S.wsum[w];
        if (w < wave) off += x;
        tot += x;
    }
    BZE_SYNC();
    total = tot;
    return off + incl - v;
}
// Inclusive maximum of v over the threads up to this one; total = the maximum of all.  Ends with a barrier.
BZE_FN uint32_t bze_scan_max(BzeShared &S, const int tid, const uint32_t v, uint32_t &total) {
    const int lane = tid % BZE_WAVE, wave = tid / BZE_WAVE;
    uint32_t incl = v;
    for (int d = 1; d < BZE_WAVE; d <<= 1) {
        const uint32_t up = (uint32_t)BZE_SHFL_UP(incl, d);
        if (lane >= d && up > incl) incl = up;
    }
    if (lane == BZE_WAVE - 1) S.wsum[wave] = incl;
    BZE_SYNC();
    uint32_t tot = 0;
    for (int w = 0; w < BZE_NW; ++w) {
        const uint32_t x = S.wsum[w];
        if (w < wave && x > incl) incl = x;
        if (x > tot) tot = x;
    }
    BZE_SYNC();
    total = tot;
    return incl;
}

// S.base = where the first key of each digit goes, from the digits digit(i), i < n (any order: the counts alone matter).
template <class Digit>
BZE_FN void bze_bins(BzeShared &S, const int tid, const uint32_t n, Digit digit) {
    for (int d = tid; d < 256; d += BZE_T) S.hist[d] = 0;
    BZE_SYNC();
    for (uint32_t i = tid; i < n; i += BZE_T) BZE_LDS_ADD(&S.hist[digit(i)], 1u);
    BZE_SYNC();
    uint32_t carry = 0;
    for (int d0 = 0; d0 < 256; d0 += BZE_T) {
        const int d = d0 + tid;
        uint32_t total;
        const uint32_t at = carry + bze_scan_add(S, tid, d < 256 ? S.hist[d] : 0u, total);
        if (d < 256) S.base[d] = at;
        carry += total;
    }
    BZE_SYNC();
}

// One stable pass of the radix sort: out[place] = item(k) for k < n in order, keyed by digit(item(k)) < 256, from the bin starts in S.base.
// Tiles of BZE_T keys go in order; inside a tile a key's place is its bin's start, the same digit's keys in the waves before, and its rank
// among the equal keys of its wave.
template <class Item, class Digit>
BZE_FN void bze_scatter(BzeShared &S, const int tid, const uint32_t n, Item item, Digit digit, uint32_t *out) {
    const int lane = tid % BZE_WAVE, wave = tid / BZE_WAVE;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int d = lane; d < 256; d += BZE_WAVE) S.wcnt[wave][d] = 0;
    BZE_SYNC();
    for (uint32_t k0 = 0; k0 < n; k0 += BZE_T) {
        const uint32_t k = k0 + tid;
        const bool live = k < n;
        const uint32_t it = live ? item(k) : 0u, d = live ? digit(it) : 0u;
        unsigned long long peers = BZE_BALLOT(live);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const unsigned long long m = BZE_BALLOT((d >> b) & 1u);
            peers &= ((d >> b) & 1u) ? m : ~m;
        }
        const uint32_t r = (uint32_t)__builtin_popcountll(peers & below);
        if (live && r == 0) S.wcnt[wave][d] = (uint32_t)__builtin_popcountll(peers);
        BZE_SYNC();
        if (live) {
            uint32_t at = S.base[d] + r;
            for (int w = 0; w < wave; ++w) at += S.wcnt[w][d];
            out[at] = it;
        }
        BZE_SYNC();
        for (int x = tid; x < 256; x += BZE_T) {
            uint32_t c = 0;
            for (int w = 0; w < BZE_NW; ++w) {
                c += S.wcnt[w][x];
                S.wcnt[w][x] = 0;
            }
            S.base[x] += c;
        }
        BZE_SYNC();
    }
}

// The stable LSD radix sort of the sequence item(k), k < n, by rank[item] < n: passes of 8 bits through a and b -> where the result lies.
template <class Item>
BZE_FN uint32_t *bze_sort_by_rank(BzeShared &S, const int tid, const uint32_t n, const uint32_t *rank, Item item, uint32_t *a, uint32_t *b) {
    int bits = 1;
    while (bits < 32 && ((n - 1) >> bits)) ++bits;
    uint32_t *from = a, *to = b;
    for (int shift = 0; shift < bits; shift += 8) {
        bze_bins(S, tid, n, [&](uint32_t i) { return (rank[i] >> shift) & 255u; });
        auto digit = [&](uint32_t j) { return (rank[j] >> shift) & 255u; };
        if (shift == 0) {
            bze_scatter(S, tid, n, item, digit, to);
        } else {
            const uint32_t *src = from;
            bze_scatter(S, tid, n, [&](uint32_t k) { return src[k]; }, digit, to);
        }
        uint32_t *t = from;
        from = to;
        to = t;
    }
    return from;
}

// Code lengths of table t over alpha symbols from S.weight[t] / S.order[t] (the symbols ascending by (count, symbol), all counts positive):
// the rule of huffman_code in csrc_deflate/deflate_kernels.hip.  One thread.
BZE_FN void bze_code_lengths(BzeShared &S, const int t, const int n) {
    uint32_t *weight = S.weight[t], *num = S.num[t];
    uint16_t *parent = S.parent[t], *depth = S.depth[t];
    int li = 0, ii = n;
    for (int nw = n; nw < 2 * n - 1; ++nw) {     // two queues: on a tie between their heads the leaf goes first
        uint32_t w = 0;
        for (int k = 0; k < 2; ++k) {
            int pick;
            if (li < n && (ii >= nw || weight[li] <= weight[ii])) pick = li++;
            else pick = ii++;
            w += weight[pick];
            parent[pick] = (uint16_t)nw;
        }
        weight[nw] = w;
    }
    depth[2 * n - 2] = 0;
    for (int k = 2 * n - 3; k >= 0; --k) depth[k] = (uint16_t)(depth[parent[k]] + 1);
    for (int i = 0; i <= BZE_MAX_LEN; ++i) num[i] = 0;
    for (int k = 0; k < n; ++k) num[depth[k] < BZE_MAX_LEN ? depth[k] : BZE_MAX_LEN] += 1;
    uint32_t total = 0;
    for (int i = 1; i <= BZE_MAX_LEN; ++i) total += num[i] << (BZE_MAX_LEN - i);
    while (total > 1u << BZE_MAX_LEN) {         // at most one step for every unit above 2^17
        num[BZE_MAX_LEN] -= 1;
        int i = BZE_MAX_LEN - 1;
        while (i > 1 && num[i] == 0) --i;
        num[i] -= 1;
        num[i + 1] += 2;
        total -= 1;
    }
    int k = n;
    for (int i = 1; i <= BZE_MAX_LEN; ++i)
        for (uint32_t c = 0; c < num[i]; ++c) S.len[t][S.order[t][--k]] = (uint8_t)i;
}

struct BzeWriter {                   // one thread, most significant bit first, whole bytes to out[pos] where pos < cap
    uint8_t *out;
    int64_t cap;
    uint32_t pos;
    uint64_t acc;
    int nb;
};
BZE_FN void bze_put(BzeWriter &w, uint32_t v, int k) {   // k <= 32
    w.acc = (w.acc << k) | v;
    w.nb += k;
    while (w.nb >= 8) {
        if ((int64_t)w.pos < w.cap) w.out[w.pos] = (uint8_t)(w.acc >> (w.nb - 8));
        ++w.pos;
        w.nb -= 8;
    }
}

#define BZE_TABLE_THREAD(t) (((t) * BZE_WAVE) % BZE_T)

// One stream: src[0, n) -> out[0, cap) through the work slot `work` (16-byte aligned, bze_layout(bze_block_cap(n, level)).bytes long).
// -> bytes written.  The blocks are coded one after the other, the bit position and the combined CRC carried from one to the next.
// cap >= bze_bound(n, level) is the caller's to check; no byte is stored at or past cap whatever it is.
BZE_FN int64_t bzip2_stream(BzeShared &S, const int tid, const uint8_t *__restrict__ stream_src, const int64_t n64, const int level,
                            uint8_t *__restrict__ out, const int64_t cap, uint8_t *work) {
    const uint32_t stream_n = (uint32_t)n64;
    const int64_t limit = bze_block_limit(level);
    const int lane = tid % BZE_WAVE;
    (void)lane;
    const int64_t block_cap = bze_block_cap(n64, level);
    const BzeLayout lay = bze_layout(block_cap);
    uint32_t *sa = (uint32_t *)(work + lay.sa), *sa2 = (uint32_t *)(work + lay.sa2);
    uint32_t *rank = (uint32_t *)(work + lay.rank), *rank2 = (uint32_t *)(work + lay.rank2);
    uint8_t *rle = work + lay.rle, *last = work + lay.last, *sel = work + lay.sel, *lists = work + lay.lists, *states = work + lay.states;
    uint16_t *sym = (uint16_t *)(work + lay.sym);

    for (int i = tid; i < 256; i += BZE_T) {
        uint32_t r = (uint32_t)i << 24;
        for (int k = 0; k < 8; ++k) r = (r << 1) ^ (0x04C11DB7u & (0u - (r >> 31)));
        S.crc_tab[i] = r;
    }
    for (int i = tid; i < 16; i += BZE_T) S.scal[i] = 0;
    BZE_SYNC();

    if (tid == 0) {
        BzeWriter w = {out, cap, 0u, 0ull, 0};
        bze_put(w, 0x425A68u, 24);
        bze_put(w, 0x30u + (uint32_t)level, 8);
        S.scal[BZE_S_POS] = w.pos;       // 4, and no partial byte
    }
    uint32_t combined = 0, sp = 0;
    const uint32_t max_blocks = (uint32_t)(((int64_t)stream_n + stream_n / 4 + limit - 5) / (limit - 4));   // a cut loses at most 4 bytes
    for (uint32_t blk = 0; blk < max_blocks && sp < stream_n; ++blk) {
        BZE_SYNC();                          // the block before is done with the shared block
        if (tid == 0) S.scal[BZE_S_CRC] = 0;
        for (int i = tid; i < 258; i += BZE_T) S.freq[i] = 0;
        BZE_SYNC();
        const uint8_t *src = stream_src + sp;
        uint32_t nblock = 0, n;
        {
            // ---- RLE1, the block cut and the CRC.  Thread t takes src[a, b).  The run a byte stands in began r0 bytes before a: the equal
            // bytes at the end of the chunks before, as far as they are of one value.  A byte at place q of its sub-run (runs cut at 255) is
            // copied when q < 4, and the sub-run's last byte, when q >= 3, is followed by the count q - 3.  First the count over what is left
            // of the stream (no further than a block can reach: 255 raw bytes give 5 bytes or more); if that is more than a block, every thread
            // notes the last sub-run end of its chunk that is still within the limit, the furthest of them is the cut, and the count is
            // made again over the block alone.  A block begins where a sub-run begins, so the run's place is counted from there.
            const uint32_t rem = stream_n - sp;
            const uint64_t span = 51ull * (uint64_t)(limit + 5) + 255ull;
            n = rem < span ? rem : (uint32_t)span;
            uint32_t chunk = 0, a = 0, b = 0, r0 = 0, at = 0;
            // mode 0: count; 1: write at rle[o ..); 2: -> where the last sub-run ends whose bytes, from o on, stay within the limit (0: none)
            auto walk = [&](const int mode, const uint32_t o) -> uint32_t {
                uint32_t run = r0, cnt = 0, prev = 0, best = 0;
                for (uint32_t x = a; x < b; ++x) {
                    const uint32_t v = src[x];
                    if (x > a && v != prev) run = 0;
                    const uint32_t q = run % 255u;
                    ++run;
                    const bool end = q == 254u || x + 1 == n || src[x + 1] != v;
                    if (q < 4u) {
                        if (mode == 1) rle[o + cnt] = (uint8_t)v;
                        ++cnt;
                    }
                    if (end && q >= 3u) {
                        if (mode == 1) rle[o + cnt] = (uint8_t)(q - 3u);
                        ++cnt;
                    }
                    if (mode == 2 && end && (int64_t)o + cnt <= limit) best = x + 1;
                    prev = v;
                }
                return mode == 2 ? best : cnt;
            };
            for (int attempt = 0; attempt < 2; ++attempt) {
                chunk = (n + BZE_T - 1) / BZE_T;
                a = (uint32_t)tid * (uint64_t)chunk < n ? tid * chunk : n;
                b = n - a < chunk ? n : a + chunk;
                uint32_t tl = 0;
                if (b > a) {
                    const uint8_t v = src[b - 1];
                    uint32_t x = b - 1;
                    while (x > a && src[x - 1] == v) --x;
                    tl = b - x;
                }
                S.tail[tid] = tl;
                BZE_SYNC();
                r0 = 0;
                if (b > a) {
                    const uint8_t v = src[a];
                    for (int c = tid - 1; c >= 0; --c) {
                        if (src[(uint32_t)c * chunk + chunk - 1] != v) break;
                        r0 += S.tail[c];
                        if (S.tail[c] < chunk) break;
                    }
                }
                uint32_t total;
                at = bze_scan_add(S, tid, walk(0, 0), total);
                nblock = total;
                if ((int64_t)total <= limit) break;
                uint32_t cut;                // the first sub-run alone is within the limit, so there is one
                bze_scan_max(S, tid, walk(2, at), cut);
                n = cut;
            }
            walk(1, at);
            uint32_t reg = tid == 0 ? 0xFFFFFFFFu : 0u;
            for (uint32_t x = a; x < b; ++x) reg = (reg << 8) ^ S.crc_tab[(reg >> 24) ^ src[x]];
            // reg(A ++ B) = reg(A) * x^(8 |B|) + reg0(B): every thread's register times x^(8 * the bytes behind its chunk), summed
            if (b > a || tid == 0) BZE_LDS_XOR(&S.scal[BZE_S_CRC], bze_gf_mul(reg, bze_gf_pow8(n - b)));
            BZE_SYNC();
        }
        const uint32_t block_crc = ~S.scal[BZE_S_CRC];

        uint32_t nmtf = 0, nsel = 0;
        int nt = 0, alpha = 0;
        {
            const uint32_t nb = nblock;
            // ---- the rotations by first byte: a stable counting sort; a rotation's rank is where its bucket starts
            bze_bins(S, tid, nb, [&](uint32_t i) { return (uint32_t)rle[i]; });
            if (tid == 0) {
                uint32_t used = 0;
                for (int v = 0; v < 256; ++v) {
                    const uint32_t end = v < 255 ? S.base[v + 1] : nb;
                    if (end > S.base[v]) {
                        S.seq[used] = (uint8_t)v;
                        S.unseq[v] = (uint8_t)used;
                        ++used;
                    }
                }
                S.scal[BZE_S_NUSED] = used;
            }
            for (uint32_t i = tid; i < nb; i += BZE_T) rank[i] = S.base[rle[i]];
            BZE_SYNC();
            const uint32_t nused = S.scal[BZE_S_NUSED];
            bze_scatter(S, tid, nb, [&](uint32_t k) { return k; }, [&](uint32_t k) { return (uint32_t)rle[k]; }, sa);
            // ---- prefix doubling: sa is in h-order and rank[i] is the first place of i's group.  j = sa[k] - h runs through the rotations in
            // the order of their second halves, so one stable sort by rank[j] gives the 2h-order.
            bool distinct = nused == nb;
            uint32_t h = 1;
            for (int round = 0; round < BZE_MAX_ROUNDS && !distinct && h < nb; ++round) {
                const uint32_t *cur = sa;
                uint32_t *res = bze_sort_by_rank(S, tid, nb, rank, [&](uint32_t k) { const uint32_t x = cur[k]; return x >= h ? x - h : x + nb - h; },
                                                 sa, sa2);     // the first pass reads sa and writes sa2: the passes alternate
                if (tid == 0) S.scal[BZE_S_NFLAG] = 0;
                uint32_t carry = 0, flags = 0;
                for (uint32_t k0 = 0; k0 < nb; k0 += BZE_T) {
                    const uint32_t k = k0 + tid;
                    uint32_t v = 0, j = 0;
                    if (k < nb) {
                        j = res[k];
                        bool f = k == 0;
                        if (!f) {
                            const uint32_t jp = res[k - 1];
                            const uint32_t j2 = j + h >= nb ? j + h - nb : j + h, jp2 = jp + h >= nb ? jp + h - nb : jp + h;
                            f = rank[j] != rank[jp] || rank[j2] != rank[jp2];
                        }
                        if (f) v = k, ++flags;
                    }
                    uint32_t top;
                    const uint32_t r = bze_scan_max(S, tid, v, top);
                    if (k < nb) rank2[j] = r > carry ? r : carry;
                    if (top > carry) carry = top;
                }
                BZE_LDS_ADD(&S.scal[BZE_S_NFLAG], flags);
                BZE_SYNC();
                distinct = S.scal[BZE_S_NFLAG] == nb;
                BZE_SYNC();
                uint32_t *t = rank;
                rank = rank2;
                rank2 = t;
                if (res != sa) {
                    sa2 = sa;
                    sa = res;
                }
                h <<= 1;
            }
            if (!distinct) {     // equal rotations (a periodic block) go by ascending start: the rotations 0, 1, 2, ... sorted stably by rank
                uint32_t *res = bze_sort_by_rank(S, tid, nb, rank, [&](uint32_t k) { return k; }, sa, sa2);
                if (res != sa) {
                    sa2 = sa;
                    sa = res;
                }
            }
            for (uint32_t k = tid; k < nb; k += BZE_T) {
                const uint32_t x = sa[k];
                last[k] = rle[x ? x - 1 : nb - 1];
                if (x == 0) S.scal[BZE_S_ORIG] = k;
            }
            BZE_SYNC();

            // ---- move to front, by chunks: each chunk's recency list (its values, the latest first); a chunk starts from the lists of the
            // chunks before it, the nearest first, then the values never seen, ascending; then every chunk runs from its true start.
            uint32_t clen = (nb + BZE_T - 1) / BZE_T;
            if (clen < BZE_MTF_CHUNK) clen = BZE_MTF_CHUNK;
            const uint32_t nchunk = (nb + clen - 1) / clen;
            const bool mine = (uint32_t)tid < nchunk;
            const uint32_t a = mine ? tid * clen : nb, b = mine && nb - a > clen ? a + clen : nb;
            uint8_t *list = lists + 256 * (mine ? tid : 0), *st = states + 256 * (mine ? tid : 0);
            if (mine) {
                uint32_t seen[8] = {0, 0, 0, 0, 0, 0, 0, 0}, len = 0;
                for (uint32_t x = b; x > a; --x) {
                    const uint32_t v = S.unseq[last[x - 1]];
                    if (!((seen[v >> 5] >> (v & 31)) & 1u)) {
                        seen[v >> 5] |= 1u << (v & 31);
                        list[len++] = (uint8_t)v;
                    }
                }
                S.tail[tid] = len;
            }
            BZE_SYNC();
            uint32_t ztail = 0;
            if (mine) {
                uint32_t seen[8] = {0, 0, 0, 0, 0, 0, 0, 0}, pos = 0;
                for (int c = tid - 1; c >= 0 && pos < nused; --c) {
                    const uint32_t len = S.tail[c];
                    for (uint32_t i = 0; i < len; ++i) {
                        const uint32_t v = lists[256 * c + i];
                        if (!((seen[v >> 5] >> (v & 31)) & 1u)) {
                            seen[v >> 5] |= 1u << (v & 31);
                            st[pos++] = (uint8_t)v;
                        }
                    }
                }
                for (uint32_t v = 0; v < nused && pos < nused; ++v)
                    if (!((seen[v >> 5] >> (v & 31)) & 1u)) st[pos++] = (uint8_t)v;
                for (uint32_t x = a; x < b; ++x) {
                    const uint8_t v = S.unseq[last[x]];
                    uint32_t p = 0;
                    uint8_t carry = st[0];
                    while (carry != v && p < 255u) { // v is one of the nused values of the list
                        ++p;
                        const uint8_t nx = st[p];
                        st[p] = carry;
                        carry = nx;
                    }
                    st[0] = v;
                    last[x] = (uint8_t)p;
                    ztail = p ? 0 : ztail + 1;
                }
            }
            BZE_SYNC();          // the lists' lengths are read
            if (mine) S.tail[tid] = ztail;
            BZE_SYNC();
            // ---- RLE2: a run of zero ranks leaves as its digits (bijective base 2, low digit first) before the next other rank or the end
            // symbol; the thread that owns that rank or the end writes them.  z0: the zeros that end the chunks before.
            uint32_t z0 = 0;
            if (mine)
                for (int c = tid - 1; c >= 0; --c) {
                    z0 += S.tail[c];
                    if (S.tail[c] < clen) break;
                }
            auto symbols = [&](const bool write, uint32_t o) -> uint32_t {
                uint32_t run = z0, cnt = 0;
                for (uint32_t x = a; x <= b; ++x) {
                    uint32_t r;
                    if (x < b) r = last[x];
                    else if (mine && b == nb) r = nused;    // the end symbol, nused + 1
                    else break;
                    if (r == 0) {
                        ++run;
                        continue;
                    }
                    if (write) {
                        for (; run; run = (run - 1) >> 1) {
                            const uint32_t d = (run & 1u) ? 0u : 1u;
                            sym[o + cnt++] = (uint16_t)d;
                            BZE_LDS_ADD(&S.freq[d], 1u);
                        }
                        sym[o + cnt++] = (uint16_t)(r + 1);
                        BZE_LDS_ADD(&S.freq[r + 1], 1u);
                    } else {
                        cnt += (run ? 31 - __builtin_clz(run + 1) : 0) + 1;
                        run = 0;
                    }
                }
                return cnt;
            };
            uint32_t total;
            const uint32_t cnt = symbols(false, 0);
            const uint32_t at = bze_scan_add(S, tid, cnt, total);
            nmtf = total;
            symbols(true, at);
            BZE_SYNC();

            // ---- the tables
            alpha = (int)nused + 2;
            nt = nmtf < 200 ? 2 : nmtf < 600 ? 3 : nmtf < 1200 ? 4 : nmtf < 2400 ? 5 : 6;
            nsel = (nmtf + BZE_GROUP - 1) / BZE_GROUP;
            if (tid == 0) {
                uint32_t rem = nmtf;
                int gs = 0;
                for (int t = nt; t >= 1; --t) {
                    const uint32_t tf = rem / t;
                    int ge = gs - 1;
                    uint32_t af = 0;
                    while (af < tf && ge < alpha - 1) af += S.freq[++ge];
                    if (ge > gs && t != nt && t != 1 && ((nt - t) & 1)) af -= S.freq[ge--];
                    for (int v = 0; v < alpha; ++v) S.len[t - 1][v] = v >= gs && v <= ge ? 0 : 15;
                    gs = ge + 1;
                    rem -= af;
                }
            }
            BZE_SYNC();
            for (int pass = 0; pass < BZE_PASSES; ++pass) {
                for (int i = tid; i < 6 * 258; i += BZE_T) S.rfreq[i / 258][i % 258] = 0;
                BZE_SYNC();
                for (uint32_t g = tid; g < nsel; g += BZE_T) {
                    const uint32_t lo = g * BZE_GROUP, hi = nmtf - lo < BZE_GROUP ? nmtf : lo + BZE_GROUP;
                    uint32_t cost[6] = {0, 0, 0, 0, 0, 0};
                    for (uint32_t i = lo; i < hi; ++i) {
                        const uint32_t s = sym[i];
#pragma unroll
                        for (int t = 0; t < 6; ++t) cost[t] += S.len[t][s];
                    }
                    int best = 0;
#pragma unroll
                    for (int t = 1; t < 6; ++t)
                        if (t < nt && cost[t] < cost[best]) best = t;
                    sel[g] = (uint8_t)best;
                    for (uint32_t i = lo; i < hi; ++i) BZE_LDS_ADD(&S.rfreq[best][sym[i]], 1u);
                }
                BZE_SYNC();
                for (int i = tid; i < nt * alpha; i += BZE_T) {      // rank sort by (count, symbol), every count at least 1
                    const int t = i / alpha, s = i % alpha;
                    const uint32_t fs = S.rfreq[t][s] ? S.rfreq[t][s] : 1u;
                    int r = 0;
                    for (int u = 0; u < alpha; ++u) {
                        const uint32_t fu = S.rfreq[t][u] ? S.rfreq[t][u] : 1u;
                        r += fu < fs || (fu == fs && u < s);
                    }
                    S.order[t][r] = (uint16_t)s;
                    S.weight[t][r] = fs;
                }
                BZE_SYNC();
                for (int t = 0; t < nt; ++t)
                    if (tid == BZE_TABLE_THREAD(t)) bze_code_lengths(S, t, alpha);
                BZE_SYNC();
            }
            for (int t = 0; t < nt; ++t)
                if (tid == BZE_TABLE_THREAD(t)) {    // canonical codes, ascending symbol within a length
                    uint32_t next[BZE_MAX_LEN + 2], c = 0;
                    for (int b2 = 1; b2 <= BZE_MAX_LEN; ++b2) {
                        next[b2] = c;
                        c = (c + S.num[t][b2]) << 1;
                    }
                    for (int s = 0; s < alpha; ++s) {
                        const uint32_t l = S.len[t][s];
                        S.code[t][s] = l << 24 | next[l]++;
                    }
                }
            BZE_SYNC();
        }

        // ---- emit: the headers by one thread, then the symbols BZE_T * BZE_EMIT_ITEMS at a time through the stage
        if (tid == 0) {
            const uint32_t cb0 = S.scal[BZE_S_CB];
            BzeWriter w = {out, cap, S.scal[BZE_S_POS], (uint64_t)(S.scal[BZE_S_CARRY] >> (8 - cb0)), (int)cb0};
            {
                bze_put(w, 0x314159u, 24);
                bze_put(w, 0x265359u, 24);
                bze_put(w, block_crc, 32);
                bze_put(w, 0u, 1);
                bze_put(w, S.scal[BZE_S_ORIG], 24);
                const int nused = alpha - 2;
                uint32_t rows[16], top = 0;
                for (int r = 0; r < 16; ++r) rows[r] = 0;
                for (int i = 0; i < nused; ++i) rows[S.seq[i] >> 4] |= 0x8000u >> (S.seq[i] & 15);
                for (int r = 0; r < 16; ++r)
                    if (rows[r]) top |= 0x8000u >> r;
                bze_put(w, top, 16);
                for (int r = 0; r < 16; ++r)
                    if (rows[r]) bze_put(w, rows[r], 16);
                bze_put(w, (uint32_t)nt, 3);
                bze_put(w, nsel, 15);
                uint32_t order = 0x543210u;          // the tables' move-to-front list, a nibble each
                for (uint32_t g = 0; g < nsel; ++g) {
                    const uint32_t t = sel[g];
                    uint32_t j = 0;
                    while (j < 5u && ((order >> (4 * j)) & 15u) != t) ++j;     // t < 6 is in the list
                    const uint32_t low = order & ((1u << (4 * j)) - 1u);
                    order = (order & ~((1u << (4 * j + 4)) - 1u)) | low << 4 | t;
                    bze_put(w, (1u << (j + 1)) - 2u, (int)j + 1);
                }
                for (int t = 0; t < nt; ++t) {
                    uint32_t cur = S.len[t][0];
                    bze_put(w, cur, 5);
                    for (int s = 0; s < alpha; ++s) {
                        const uint32_t l = S.len[t][s];
                        for (; cur < l; ++cur) bze_put(w, 2u, 2);
                        for (; cur > l; --cur) bze_put(w, 3u, 2);
                        bze_put(w, 0u, 1);
                    }
                }
            }
            S.scal[BZE_S_POS] = w.pos;
            S.scal[BZE_S_CB] = (uint32_t)w.nb;
            S.scal[BZE_S_CARRY] = (uint32_t)(w.acc & ((1u << w.nb) - 1u)) << (8 - w.nb);    // the partial byte, its bits at the top
        }
        BZE_SYNC();
        uint32_t opos = S.scal[BZE_S_POS], cb = S.scal[BZE_S_CB], carry = S.scal[BZE_S_CARRY];
        for (uint32_t base = 0; base < nmtf; base += BZE_T * BZE_EMIT_ITEMS) {
            BZE_SYNC();
            for (int k = tid; k < BZE_STAGE_WORDS; k += BZE_T) S.stage[k] = k == 0 ? carry << 24 : 0u;
            BZE_SYNC();
            uint32_t v[BZE_EMIT_ITEMS], nbit[BZE_EMIT_ITEMS], sum = 0;
#pragma unroll
            for (int j = 0; j < BZE_EMIT_ITEMS; ++j) {
                const uint32_t i = base + BZE_EMIT_ITEMS * tid + j;
                v[j] = 0, nbit[j] = 0;
                if (i < nmtf) {
                    const uint32_t c = S.code[sel[i / BZE_GROUP]][sym[i]];
                    v[j] = c & 0xFFFFFFu, nbit[j] = c >> 24;
                }
                sum += nbit[j];
            }
            uint32_t total;
            uint32_t pos = cb + bze_scan_add(S, tid, sum, total);
#pragma unroll
            for (int j = 0; j < BZE_EMIT_ITEMS; ++j) {
                if (nbit[j]) {
                    const uint32_t w = pos >> 5, end = (pos & 31u) + nbit[j];   // bit p of the step is bit 31 - (p & 31) of word p >> 5
                    if (end <= 32u) {
                        BZE_LDS_OR(&S.stage[w], v[j] << (32u - end));
                    } else {
                        BZE_LDS_OR(&S.stage[w], v[j] >> (end - 32u));
                        BZE_LDS_OR(&S.stage[w + 1], v[j] << (64u - end));
                    }
                    pos += nbit[j];
                }
            }
            BZE_SYNC();
            const uint32_t tot = cb + total, nbytes = tot >> 3;
            for (uint32_t x = tid; x < nbytes; x += BZE_T)
                if ((int64_t)opos + x < cap) out[opos + x] = (uint8_t)(S.stage[x >> 2] >> (24u - 8u * (x & 3u)));
            carry = (S.stage[nbytes >> 2] >> (24u - 8u * (nbytes & 3u))) & 255u;
            cb = tot & 7u;
            opos += nbytes;
        }
        BZE_SYNC();
        if (tid == 0) {
            S.scal[BZE_S_POS] = opos;
            S.scal[BZE_S_CB] = cb;
            S.scal[BZE_S_CARRY] = carry;
        }
        combined = (combined << 1 | combined >> 31) ^ block_crc;
        sp += n;
    }
    BZE_SYNC();
    if (tid == 0) {
        const uint32_t cb = S.scal[BZE_S_CB];
        BzeWriter w = {out, cap, S.scal[BZE_S_POS], (uint64_t)(S.scal[BZE_S_CARRY] >> (8 - cb)), (int)cb};
        bze_put(w, 0x177245u, 24);
        bze_put(w, 0x385090u, 24);
        bze_put(w, combined, 32);
        if (w.nb) bze_put(w, 0u, 8 - w.nb);
        S.scal[BZE_S_POS] = w.pos;
    }
    BZE_SYNC();
    return (int64_t)S.scal[BZE_S_POS];
}

#endif  // RPCC_BZIP2_CORE_H
