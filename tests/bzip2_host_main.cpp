// The encoder of csrc_bzip2/bzip2_core.h as a host program with a workgroup of one thread (tests/test_bzip2_core_host.py): the same text
// the gfx950 kernel is compiled from, so the bytes it gives are the kernel's but for what the threads do in parallel.
// Input file: int64 count, then per stream int64 length, int64 level, bytes.
// Output file: per stream int64 bytes written, int64 bound, int64 work bytes, then the bytes written.
// Source, destination (bze_bound bytes) and work slot (bze_layout bytes) are heap blocks of exactly the stated sizes, so a sanitizer build
// (-fsanitize=address,undefined) sees any overrun; the work slot and the shared block are filled with 0xCD first.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "rpcc_bzip2.h"

#define BZE_FN static inline
#define BZE_HD static inline
#define BZE_T 1
#define BZE_WAVE 1
#define BZE_SYNC() ((void)0)
#define BZE_BALLOT(p) ((p) ? 1ull : 0ull)
#define BZE_SHFL_UP(v, d) (v)
#define BZE_LDS_ADD(p, v) ((void)(*(p) += (v)))
#define BZE_LDS_OR(p, v) ((void)(*(p) |= (v)))
#define BZE_LDS_XOR(p, v) ((void)(*(p) ^= (v)))
#include "bzip2_core.h"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *g = fopen(argv[2], "wb");
    int64_t n;
    if (!f || !g || fread(&n, 8, 1, f) != 1) return 2;
    static BzeShared S;
    for (int64_t i = 0; i < n; ++i) {
        int64_t len, level;
        if (fread(&len, 8, 1, f) != 1 || fread(&level, 8, 1, f) != 1) return 2;
        const int64_t cap = bze_bound(len, (int)level), wbytes = bze_layout(bze_block_cap(len, (int)level)).bytes;
        if (cap <= 0 || wbytes > bze_slots_bytes(1, len)) return 3;      // the call's bound of the slots covers the layout
        uint8_t *in = (uint8_t *)malloc(len ? len : 1), *out = (uint8_t *)malloc(cap);
        uint8_t *work = (uint8_t *)aligned_alloc(16, wbytes);
        if (fread(in, 1, len, f) != (size_t)len) return 2;
        memset(&S, 0xCD, sizeof S);   // LDS holds anything at launch
        memset(work, 0xCD, wbytes);
        const int64_t got = bzip2_stream(S, 0, in, len, (int)level, out, cap, work);
        fwrite(&got, 8, 1, g);
        fwrite(&cap, 8, 1, g);
        fwrite(&wbytes, 8, 1, g);
        if (got > cap) return 4;
        if (got > 0) fwrite(out, 1, got, g);
        free(in);
        free(out);
        free(work);
    }
    return fclose(g) ? 2 : 0;
}
