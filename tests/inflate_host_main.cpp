// The decoder of csrc_inflate/inflate_core.h as a host program with a wave of one lane (tests/test_inflate_core_host.py): the same text the
// gfx950 kernel is compiled from, so the statuses and bytes it gives are the kernel's but for what the lanes do in parallel.
// Input file: int64 count, then per stream int64 length, int64 capacity, bytes.  Output file: per stream int64 status, int64 produced, bytes if OK.
// Source and destination are heap blocks of exactly the stated sizes, so a sanitizer build (-fsanitize=address,undefined) sees any overrun.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "rpcc_inflate.h"

#define INF_FN static inline
#define INF_CONST static const
#define INF_WAVE 1
#define INF_SYNC() ((void)0)
#define INF_UNI(x) ((int)(x))
#define INF_BALLOT(p) ((p) ? 1ull : 0ull)
#define INF_SHFL_XOR(v, m) (v)
static inline uint32_t brev32(uint32_t x) {
    uint32_t r = 0;
    for (int i = 0; i < 32; ++i) r |= ((x >> i) & 1u) << (31 - i);
    return r;
}
#define INF_BREV(x) brev32(x)
#include "inflate_core.h"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *g = fopen(argv[2], "wb");
    int64_t n;
    if (!f || !g || fread(&n, 8, 1, f) != 1) return 2;
    static InfShared S;
    for (int64_t i = 0; i < n; ++i) {
        int64_t len, cap;
        if (fread(&len, 8, 1, f) != 1 || fread(&cap, 8, 1, f) != 1) return 2;
        uint8_t *in = (uint8_t *)malloc(len ? len : 1), *out = (uint8_t *)malloc(cap > 0 ? cap : 1);
        if (fread(in, 1, len, f) != (size_t)len) return 2;
        memset(&S, 0xCD, sizeof S);   // LDS holds anything at launch
        int64_t produced = -1;
        const int64_t st = inflate_stream(S, 0, in, len, out, cap, produced);
        fwrite(&st, 8, 1, g);
        fwrite(&produced, 8, 1, g);
        if (st == 0) fwrite(out, 1, produced, g);
        free(in);
        free(out);
    }
    return fclose(g) ? 2 : 0;
}
