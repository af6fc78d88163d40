// csrc_rans/rans_core.h with csrc_rans/rans_filter.h -- version 2 of the 'rans' format, the delta filter -- as a host program with the wave
// emulated lane by lane (tests/test_rans_filter_core_host.py), after tests/rans_host_main.cpp, which stays the version-1 program: the
// same text the gfx950 kernels are compiled from around a plain statement of the kernels' glue.  The histogram goes the kernel's way
// (dwords through rans_delta_dword, the tail through rans_delta_byte), the chunks through rans_encode_chunk_filtered, and the decoder's
// storing pass is rans_decode_chunk followed by rans_unfilter_chunk over the chunk it stored.
// Input file: int64 count, then per row int64 op and
//   op 0 (encode): int64 length, width, chunk_log2, fallback, filter; bytes   -> int64 length, bytes
//   op 1 (decode): int64 length, capacity; bytes                              -> int64 status, produced; bytes if OK
// Sources and destinations are heap blocks of exactly the stated sizes, so a sanitizer build (-fsanitize=address,undefined) sees any overrun.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rpcc_rans.h"

#define RANS_FN static inline
#define RANS_NL 64
#define RANS_EACH(l) for (int l = 0; l < 64; ++l)
#define RANS_AT(a, l) a[l]
template <class T>
static inline uint64_t ballot64(const T *a) {
    uint64_t m = 0;
    for (int l = 0; l < 64; ++l) m |= (uint64_t)(a[l] != 0) << l;
    return m;
}
static inline uint64_t sum64(const uint64_t *a) {
    uint64_t s = 0;
    for (int l = 0; l < 64; ++l) s += a[l];
    return s;
}
static inline uint32_t max32(const uint32_t *a) {
    uint32_t m = 0;
    for (int l = 0; l < 64; ++l) m = a[l] > m ? a[l] : m;
    return m;
}
static inline void scan32(uint32_t *a) {
    for (int l = 1; l < 64; ++l) a[l] += a[l - 1];
}
#define RANS_BALLOT(a) ballot64(a)
#define RANS_SUM64(a) sum64(a)
#define RANS_MAX32(a) max32(a)
#define RANS_SCAN32(a) scan32(a)
#define RANS_LAST32(a) ((a)[63])
#define RANS_SYNC() ((void)0)
#include "rans_core.h"

static std::vector<uint8_t> encode(const uint8_t *src, uint32_t n, uint32_t width, uint32_t clog, bool fallback, uint32_t filter) {
    std::vector<uint8_t> stored(RANS_HEADER + n);
    rans_put_header(stored.data(), 0, width, n, clog);
    if (n) memcpy(stored.data() + RANS_HEADER, src, n);
    if (n == 0) return stored;
    std::vector<uint8_t> out(RANS_HEADER);
    if (filter != RANS_FILTER_NONE) rans_put_header_filtered(out.data(), width, n, clog, filter);
    else rans_put_header(out.data(), 1, width, n, clog);
    const uint32_t size = 1u << clog, nch = (n + size - 1) / size;
    uint32_t counts[4][256] = {{0}};
    for (uint32_t c = 0; c < nch; ++c) {         // hist_kernel's loads
        const uint8_t *s = src + (size_t)c * size;
        const uint32_t k = n - c * size < size ? n - c * size : size;
        for (uint32_t x = 0; x + 4 <= k; x += 4) {
            uint32_t v = rans_ld32(s + x);
            if (filter == RANS_FILTER_DELTA) v = rans_delta_dword(v, x ? rans_ld_elem(s + x - width, width) : 0u, width);
            for (uint32_t j = 0; j < 4; ++j) ++counts[j & (width - 1)][(v >> (8 * j)) & 255u];
        }
        for (uint32_t x = k & ~3u; x < k; ++x) ++counts[x & (width - 1)][filter == RANS_FILTER_DELTA ? rans_delta_byte(s, x, k, width) : s[x]];
    }
    std::vector<uint32_t> enc(width * 512);
    for (uint32_t p = 0; p < width; ++p) {
        uint16_t freq[256] = {0};
        const uint32_t total = rans_plane_bytes(n, width, p);
        if (total) rans_normalise(0, counts[p], total, freq);
        uint32_t m = 0, cum = 0;
        for (int s = 0; s < 256; ++s) m += freq[s] != 0;
        out.push_back((uint8_t)m), out.push_back((uint8_t)(m >> 8));
        for (int s = 0; s < 256; ++s) {
            if (!freq[s]) continue;
            out.push_back((uint8_t)s), out.push_back((uint8_t)(freq[s] - 1)), out.push_back((uint8_t)((freq[s] - 1) >> 8));
            rans_enc_entry(freq[s], cum, &enc[(p * 256 + s) * 2]);
            cum += freq[s];
        }
    }
    const size_t dir = out.size();
    out.resize(dir + 4 * (size_t)nch);
    for (uint32_t c = 0; c < nch; ++c) {
        const uint32_t k = n - c * size < size ? n - c * size : size;
        std::vector<uint8_t> chunk(src + (size_t)c * size, src + (size_t)c * size + k);   // a block of its own: a read in front of the chunk is an overrun
        std::vector<uint8_t> slot(2 * (size_t)k + 256);
        const uint32_t len = rans_encode_chunk_filtered(0, chunk.data(), k, width, filter, enc.data(), slot.data() + slot.size());
        rans_st32(out.data() + dir + 4 * (size_t)c, len);
        out.insert(out.end(), slot.end() - len, slot.end());
    }
    return out.size() < stored.size() || !fallback ? out : stored;
}

static int decode(const uint8_t *in, int64_t len, uint8_t *dst, int64_t cap, int64_t &produced) {
    RansInfo I;
    produced = 0;
    int st = rans_parse(0, in, len, cap, I);
    if (st != RPCC_RANS_OK) return st;
    if (I.mode == 0) {
        if (I.filter != RANS_FILTER_NONE) abort();   // rans_parse accepts no stored 'RB' stream
        if (I.n) memcpy(dst, in + RANS_HEADER, I.n);
        produced = I.n;
        return RPCC_RANS_OK;
    }
    RansInfo J;
    rans_read_header(in, RANS_HEADER, J);            // the chunk kernels' way to the same places
    rans_layout(in, J);
    if (J.dir != I.dir || J.pay != I.pay || J.nch != I.nch || J.filter != I.filter) abort();
    std::vector<uint8_t> lookup(I.width * RANS_PROB);
    std::vector<uint32_t> fc(I.width * 256);
    for (uint32_t p = 0; p < I.width; ++p) {
        uint32_t cum = 0;
        for (uint32_t e = 0; e < I.m[p]; ++e) {
            const uint8_t *q = in + I.tab[p] + 3 * e;
            const uint32_t f = rans_ld16(q + 1) + 1;
            fc[p * 256 + q[0]] = rans_dec_entry(f, cum);
            memset(&lookup[p * RANS_PROB + cum], q[0], f);
            cum += f;
        }
    }
    std::vector<uint32_t> ring(RANS_RING / 2, 0xCDCDCDCDu);
    const uint32_t size = 1u << I.chunk_log2;
    for (int pass = 0; pass < 2; ++pass) {       // the check, then the stores
        for (uint32_t c = 0; c < I.nch; ++c) {
            const uint32_t k = I.n - c * size < size ? I.n - c * size : size;
            const int64_t at = rans_chunk_offset(0, in, I, c);
            const int cs = rans_decode_chunk(0, in + at, rans_ld32(in + I.dir + 4 * (int64_t)c), k, I.width, lookup.data(), fc.data(), ring.data(),
                                             pass ? dst + (size_t)c * size : nullptr);
            if (pass && I.filter == RANS_FILTER_DELTA) rans_unfilter_chunk(0, dst + (size_t)c * size, k, I.width);
            st = cs < st ? cs : st;
        }
        if (st != RPCC_RANS_OK) return st;
    }
    produced = I.n;
    return RPCC_RANS_OK;
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *g = fopen(argv[2], "wb");
    int64_t rows;
    if (!f || !g || fread(&rows, 8, 1, f) != 1) return 2;
    for (int64_t i = 0; i < rows; ++i) {
        int64_t op, h[5];
        if (fread(&op, 8, 1, f) != 1) return 2;
        if (fread(h, 8, op == 0 ? 5 : 2, f) != (size_t)(op == 0 ? 5 : 2)) return 2;
        const int64_t len = h[0];
        uint8_t *in = (uint8_t *)malloc(len ? len : 1);
        if (fread(in, 1, len, f) != (size_t)len) return 2;
        if (op == 0) {
            const std::vector<uint8_t> s = encode(in, (uint32_t)len, (uint32_t)h[1], (uint32_t)h[2], h[3] != 0, (uint32_t)h[4]);
            const int64_t n = (int64_t)s.size();
            fwrite(&n, 8, 1, g);
            fwrite(s.data(), 1, s.size(), g);
        } else {
            const int64_t cap = h[1];
            uint8_t *out = (uint8_t *)malloc(cap > 0 ? cap : 1);
            int64_t produced = -1;
            const int64_t st = decode(in, len, out, cap, produced);
            fwrite(&st, 8, 1, g);
            fwrite(&produced, 8, 1, g);
            if (st == 0) fwrite(out, 1, produced, g);
            free(out);
        }
        free(in);
    }
    return fclose(g) ? 2 : 0;
}
