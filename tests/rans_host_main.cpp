// csrc_rans/rans_core.h as a host program with the wave emulated lane by lane (tests/test_rans_core_host.py): the same text the gfx950
// kernels are compiled from -- normalisation, parsing, the coding of a chunk with its ballots and prefix counts -- around a plain
// statement of what the kernels' own glue does (histograms, table building, assembly).
// Input file: int64 count, then per row int64 op and
//   op 0 (encode): int64 length, width, chunk_log2, fallback; bytes          -> int64 length, bytes
//   op 1 (decode): int64 length, capacity; bytes                             -> int64 status, produced; bytes if OK
//   op 2 (the exact division of rans_div): nothing                           -> int64 states checked, int64 mismatches
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
#define RANS_BALLOT(a) ballot64(a)
#define RANS_SUM64(a) sum64(a)
#define RANS_MAX32(a) max32(a)
#define RANS_SYNC() ((void)0)
#include "rans_core.h"

static std::vector<uint8_t> encode(const uint8_t *src, uint32_t n, uint32_t width, uint32_t clog, bool fallback) {
    std::vector<uint8_t> stored(RANS_HEADER + n);
    rans_put_header(stored.data(), 0, width, n, clog);
    if (n) memcpy(stored.data() + RANS_HEADER, src, n);
    if (n == 0) return stored;
    std::vector<uint8_t> out(RANS_HEADER);
    rans_put_header(out.data(), 1, width, n, clog);
    std::vector<uint32_t> enc(width * 512);
    for (uint32_t p = 0; p < width; ++p) {
        uint32_t counts[256] = {0};
        uint16_t freq[256] = {0};
        for (uint32_t i = p; i < n; i += width) ++counts[src[i]];
        const uint32_t total = rans_plane_bytes(n, width, p);
        if (total) rans_normalise(0, counts, total, freq);
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
    const uint32_t size = 1u << clog, nch = (n + size - 1) / size;
    const size_t dir = out.size();
    out.resize(dir + 4 * (size_t)nch);
    for (uint32_t c = 0; c < nch; ++c) {
        const uint32_t k = n - c * size < size ? n - c * size : size;
        std::vector<uint8_t> slot(2 * (size_t)k + 256);          // exactly the scratch slot's worst case
        const uint32_t len = rans_encode_chunk(0, src + (size_t)c * size, k, width, enc.data(), slot.data() + slot.size());
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
        if (I.n) memcpy(dst, in + RANS_HEADER, I.n);
        produced = I.n;
        return RPCC_RANS_OK;
    }
    RansInfo J = I;
    rans_layout(in, J);            // the chunk kernels' way to the same places
    if (J.dir != I.dir || J.pay != I.pay || J.nch != I.nch) abort();
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
            st = cs < st ? cs : st;
        }
        if (st != RPCC_RANS_OK) return st;
    }
    produced = I.n;
    return RPCC_RANS_OK;
}

// rans_div against the machine's division: every f in 1 .. 4096 at the states around every multiple of f that is a power of two away from
// the ends of the 32-bit range, around the encoder's renormalisation threshold and at a stride through the range.
static void check_div(int64_t &checked, int64_t &bad) {
    checked = bad = 0;
    for (uint32_t f = 1; f <= 4096; ++f) {
        const uint32_t m = rans_rcp(f), l = rans_log2_ceil(f);
        auto at = [&](uint64_t x) {
            if (x > 0xFFFFFFFFull) return;
            ++checked;
            bad += rans_div((uint32_t)x, m, l) != (uint32_t)x / f;
        };
        auto around = [&](uint64_t x) {
            const uint64_t q = x / f * f;
            for (int64_t d = -2; d <= 2; ++d) {
                if ((int64_t)q + d >= 0) at(q + d);
                at(q + f + d);
                if ((int64_t)x + d >= 0) at(x + d);
            }
        };
        for (int b = 0; b <= 32; ++b) around((1ull << b) - (b == 32));
        around((uint64_t)f << 20), around((uint64_t)f << 16), around(0xFFFFFFFFull - f);
        for (uint64_t x = 0; x <= 0xFFFFFFFFull; x += 0x00FFF1u * f + 12345u) around(x);
    }
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *g = fopen(argv[2], "wb");
    int64_t rows;
    if (!f || !g || fread(&rows, 8, 1, f) != 1) return 2;
    for (int64_t i = 0; i < rows; ++i) {
        int64_t op, h[4];
        if (fread(&op, 8, 1, f) != 1) return 2;
        if (op == 2) {
            int64_t r[2];
            check_div(r[0], r[1]);
            fwrite(r, 8, 2, g);
            continue;
        }
        if (fread(h, 8, op == 0 ? 4 : 2, f) != (size_t)(op == 0 ? 4 : 2)) return 2;
        const int64_t len = h[0];
        uint8_t *in = (uint8_t *)malloc(len ? len : 1);
        if (fread(in, 1, len, f) != (size_t)len) return 2;
        if (op == 0) {
            const std::vector<uint8_t> s = encode(in, (uint32_t)len, (uint32_t)h[1], (uint32_t)h[2], h[3] != 0);
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
