// lz_match.h -- the match finder librpcc_lz4.so (csrc_lz4/) and librpcc_deflate.so (csrc_deflate/) share: the greedy parse of
// DESIGN.md section 11, steps 1-5, for one 256-thread workgroup per stream and one tile of 1024 start positions at a time.
// The 16384-entry last-position table stays in LDS across tiles.  Per tile: the hash of every position; an LDS bitonic sort of
// (hash, position) gives each position its in-tile predecessor of the same hash, or the table's entry where it has none; the
// accept test runs for all positions and is stored as 64-bit ballots; the table takes each hash's last position of the tile.
// Wave 0 then walks the greedy parse over the ballots, extending a match 256 bytes per step with a wave-wide compare, and
// leaves the tile's sequences (at most 256: each consumes >= 4 positions of the tile) in seq[].  The only parameter is the
// largest offset a match may have: 65535 for LZ4, 32768 for deflate.
#ifndef RPCC_LZ_MATCH_H
#define RPCC_LZ_MATCH_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#define ENC_THREADS 256
#define ENC_TILE 1024                // positions per tile (local position: 10 bits of the sort key)
#define ENC_SEQ (ENC_TILE / 4)       // sequences starting in one tile
#define HASH_LOG 14
#define NONE 0xFFFFFFFFu
#define MFLIMIT 12                   // a match starts at p <= n - 12
#define LAST_LITERALS 5              // the last 5 bytes are literals

__device__ __forceinline__ uint32_t hash5(uint64_t v) {   // v: the little-endian 40-bit value of src[p..p+5)
    return (uint32_t)(((v << 24) * 889523592379ull) >> (64 - HASH_LOG));
}

__device__ __forceinline__ uint32_t ld4(const uint8_t *p) {
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

// Exclusive scan of one value per thread of a 256-thread block; *total gets the sum.  Ends with a barrier.
__device__ uint32_t block_scan256(uint32_t v, uint32_t *wsum, uint32_t *total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t x = v;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    if (lane == 63) wsum[w] = x;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (int k = 0; k < ENC_THREADS / 64; ++k) {
        before += k < w ? wsum[k] : 0;
        all += wsum[k];
    }
    *total = all;
    __syncthreads();
    return before + x - v;
}

struct MatchShared {
    uint32_t table[1 << HASH_LOG];   // last position of each hash before the tile (NONE: none)
    uint32_t keys[ENC_TILE];         // hash << 10 | local position, sorted
    uint32_t cand[ENC_TILE];         // c(p) by local position
    uint64_t acc[ENC_TILE / 64];     // accept bits
    uint4 seq[ENC_SEQ];              // literal start, literal length, offset, L
    uint8_t bytes[ENC_TILE + 4];     // src[t0 .. t0 + cnt + 4)
    uint32_t i, anchor, nseq;
};

// Positions of src[0 .. n) that may start a match: 0 .. n - 12.
__device__ __forceinline__ uint32_t match_positions(uint32_t n) { return n >= MFLIMIT ? n - MFLIMIT + 1 : 0; }

// Before the first tile.  Ends with a barrier.
__device__ __forceinline__ void match_init(MatchShared &S) {
    for (int k = threadIdx.x; k < (1 << HASH_LOG); k += ENC_THREADS) S.table[k] = NONE;
    if (threadIdx.x == 0) S.i = S.anchor = 0;
    __syncthreads();
}

// The tile of positions t0 .. t0 + cnt (cnt = min(ENC_TILE, m - t0), m = match_positions(n)): S.seq[0 .. S.nseq) are the
// sequences that start in it, S.anchor the first byte no sequence covers yet.  Ends with a barrier; the caller puts one more
// after its last use of S.seq, before the next tile.
template <uint32_t MAX_OFFSET>
__device__ __forceinline__ void match_tile(MatchShared &S, const uint8_t *__restrict__ src, uint32_t n, uint32_t t0, uint32_t cnt) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (uint32_t k = tid; k < cnt + 4; k += ENC_THREADS) S.bytes[k] = src[t0 + k];   // t0 + cnt + 3 <= n - 9
    __syncthreads();
    for (uint32_t lp = tid; lp < ENC_TILE; lp += ENC_THREADS) {
        uint32_t key = NONE;
        if (lp < cnt) {
            const uint64_t v = (uint64_t)ld4(S.bytes + lp) | (uint64_t)S.bytes[lp + 4] << 32;
            key = hash5(v) << 10 | lp;
        }
        S.keys[lp] = key;
    }
    __syncthreads();
    // bitonic sort of keys[0 .. ENC_TILE), ascending: equal hashes end up adjacent, in position order
    for (uint32_t k = 2; k <= ENC_TILE; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t q = tid; q < ENC_TILE / 2; q += ENC_THREADS) {
                const uint32_t a = 2 * j * (q / j) + (q % j), b = a + j;
                const uint32_t ka = S.keys[a], kb = S.keys[b];
                if ((ka > kb) == ((a & k) == 0)) {
                    S.keys[a] = kb;
                    S.keys[b] = ka;
                }
            }
            __syncthreads();
        }
    }
    // c(p): the previous position of the same hash inside the tile, else the table's last one before the tile
    for (uint32_t e = tid; e < cnt; e += ENC_THREADS) {
        const uint32_t key = S.keys[e], h = key >> 10, lp = key & 1023;
        const uint32_t prev = e > 0 ? S.keys[e - 1] : NONE;
        S.cand[lp] = (e > 0 && (prev >> 10) == h) ? t0 + (prev & 1023) : S.table[h];
    }
    __syncthreads();
    for (uint32_t e = tid; e < cnt; e += ENC_THREADS) {
        const uint32_t key = S.keys[e], h = key >> 10;
        if (e + 1 == cnt || (S.keys[e + 1] >> 10) != h) S.table[h] = t0 + (key & 1023);
    }
    // accept: c exists, p - c <= MAX_OFFSET, src[c..c+4) == src[p..p+4)
    for (uint32_t lp = tid; lp < ENC_TILE; lp += ENC_THREADS) {
        bool a = false;
        if (lp < cnt) {
            const uint32_t c = S.cand[lp];
            a = c != NONE && t0 + lp - c <= MAX_OFFSET && ld4(src + c) == ld4(S.bytes + lp);
        }
        const uint64_t bits = __ballot(a);
        if (lane == 0) S.acc[lp >> 6] = bits;
    }
    __syncthreads();
    // greedy walk over the accept bits (wave 0; every lane holds the same state)
    if (wave == 0) {
        uint32_t i = S.i, anchor = S.anchor, nseq = 0;
        const uint32_t end = t0 + cnt;
        while (i < end) {
            uint32_t w = (i - t0) >> 6;
            uint64_t bits = S.acc[w] & (~0ull << ((i - t0) & 63));
            while (bits == 0 && ++w < ENC_TILE / 64) bits = S.acc[w];
            if (bits == 0) {
                i = end;
                break;
            }
            const uint32_t p = t0 + w * 64 + (__ffsll((unsigned long long)bits) - 1);   // < end: bits past cnt are 0
            const uint32_t c = S.cand[p - t0];
            const uint32_t lim = n - LAST_LITERALS - p;   // L <= lim (>= 7)
            uint32_t L = 4;
            while (L < lim) {
                const uint32_t x0 = L + lane * 4;
                uint32_t mm = 4;
                for (int k = 3; k >= 0; --k)
                    if (x0 + k < lim && src[c + x0 + k] != src[p + x0 + k]) mm = k;
                const uint64_t miss = __ballot(mm < 4);
                if (miss) {
                    const int l = __ffsll((unsigned long long)miss) - 1;
                    L += l * 4 + __shfl(mm, l);
                    break;
                }
                L = min(lim, L + 256);
            }
            if (lane == 0) S.seq[nseq] = make_uint4(anchor, p - anchor, p - c, L);
            ++nseq;
            i = p + L;
            anchor = i;
        }
        if (lane == 0) {
            S.i = i;
            S.anchor = anchor;
            S.nseq = nseq;
        }
    }
    __syncthreads();
}

#endif  // RPCC_LZ_MATCH_H
