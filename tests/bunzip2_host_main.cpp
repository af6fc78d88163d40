// The decoder of csrc_bunzip2/bunzip2_core.h as a host program with a wave of one lane (tests/test_bunzip2_core_host.py): the same text the
// gfx950 kernel is compiled from, so the statuses and bytes it gives are the kernel's but for what the lanes do in parallel.
// Input file: int64 count, then per stream int64 length, int64 capacity, int64 work block length, bytes.
// Output file: per stream int64 status, int64 produced, int64 input bytes used, then the bytes if OK (with E_OVERRUN: the first `capacity`).
// Source, destination and work slot are heap blocks of exactly the stated sizes, so a sanitizer build (-fsanitize=address,undefined)
// sees any overrun; the work slot and the shared block are filled with 0xCD first.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "rpcc_bunzip2.h"

#define BZ_FN static inline
#define BZ_HD static inline
#define BZ_WAVE 1
#define BZ_SYNC() ((void)0)
#define BZ_UNI(x) ((int)(x))
#define BZ_BALLOT(p) ((p) ? 1ull : 0ull)
#define BZ_SHFL_XOR(v, m) (v)
#define BZ_SHFL_UP(v, d) (v)
#define BZ_READLANE(v, l) (v)
#define BZ_LDS_ADD(p, v) ((void)(*(p) += (v)))
static inline uint32_t fetch_add(uint32_t *p, uint32_t v) {
    const uint32_t old = *p;
    *p += v;
    return old;
}
#define BZ_LDS_FETCH_ADD(p, v) fetch_add((p), (v))
#include "bunzip2_core.h"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *g = fopen(argv[2], "wb");
    int64_t n;
    if (!f || !g || fread(&n, 8, 1, f) != 1) return 2;
    static BzShared S;
    for (int64_t i = 0; i < n; ++i) {
        int64_t len, cap, blk;
        if (fread(&len, 8, 1, f) != 1 || fread(&cap, 8, 1, f) != 1 || fread(&blk, 8, 1, f) != 1) return 2;
        const int64_t wbytes = bz_work_layout(blk).bytes;
        if (bz_work_block(wbytes) != blk) return 3;      // the layout and its inverse are one statement
        uint8_t *in = (uint8_t *)malloc(len ? len : 1), *out = (uint8_t *)malloc(cap > 0 ? cap : 1), *work = (uint8_t *)malloc(wbytes ? wbytes : 4);
        if (fread(in, 1, len, f) != (size_t)len) return 2;
        memset(&S, 0xCD, sizeof S);   // LDS holds anything at launch
        memset(work, 0xCD, wbytes ? wbytes : 4);
        int64_t produced = -1, used = -1;
        const int64_t st = bunzip2_stream(S, 0, in, len, out, cap, work, wbytes, produced, used);
        fwrite(&st, 8, 1, g);
        fwrite(&produced, 8, 1, g);
        fwrite(&used, 8, 1, g);
        if (st == RPCC_BUNZIP2_OK) fwrite(out, 1, produced, g);
        if (st == RPCC_BUNZIP2_E_OVERRUN) fwrite(out, 1, cap, g);
        free(in);
        free(out);
        free(work);
    }
    return fclose(g) ? 2 : 0;
}
