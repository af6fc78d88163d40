// The encoder of csrc_bzip2/bzip2_core.h as a host program (tests/test_bzip2_core_host.py): the same text the gfx950 kernel is compiled
// from.  By default the workgroup has one thread, so the bytes are the kernel's but for what the threads do in parallel; with
// -DHOST_T=1024 -DHOST_WAVE=64 (the test reads BZE_T and BZE_WAVE from bzip2_kernels.hip) the threads are those of tests/host_wave.h, which
// is where barriers, ballots, shuffles and the LDS atomics are run, under a thread sanitizer too.  Every thread must return the same count.
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
#ifndef HOST_T
#define HOST_T 1
#define HOST_WAVE 1
#endif
#define BZE_T HOST_T
#define BZE_WAVE HOST_WAVE
#if HOST_T == 1
#define BZE_SYNC() ((void)0)
#define BZE_BALLOT(p) ((p) ? 1ull : 0ull)
#define BZE_SHFL_UP(v, d) (v)
#define BZE_LDS_ADD(p, v) ((void)(*(p) += (v)))
#define BZE_LDS_OR(p, v) ((void)(*(p) |= (v)))
#define BZE_LDS_XOR(p, v) ((void)(*(p) ^= (v)))
#else
#define HW_T HOST_T
#define HW_WAVE HOST_WAVE
#include "host_wave.h"
#define BZE_SYNC() hw::sync(HW_AT)
#define BZE_BALLOT(p) hw::ballot((p), HW_AT)
#define BZE_SHFL_UP(v, d) hw::shfl_up((v), (d), HW_AT)
#define BZE_LDS_ADD(p, v) hw::lds_add((p), (v))
#define BZE_LDS_OR(p, v) hw::lds_or((p), (v))
#define BZE_LDS_XOR(p, v) hw::lds_xor((p), (v))
#endif
#include "bzip2_core.h"

static FILE *f, *g;
static int64_t n, len, level, cap, wbytes, got_of[HOST_T];
static uint8_t *in, *out, *work;
static BzeShared S;

// every thread runs the streams in turn; thread 0 reads, allocates and writes between two barriers
static void threads(int tid) {
    for (int64_t i = 0; i < n; ++i) {
        if (tid == 0) {
            if (fread(&len, 8, 1, f) != 1 || fread(&level, 8, 1, f) != 1) _Exit(2);
            cap = bze_bound(len, (int)level), wbytes = bze_layout(bze_block_cap(len, (int)level)).bytes;
            if (cap <= 0 || wbytes > bze_slots_bytes(1, len)) _Exit(3);      // the call's bound of the slots covers the layout
            in = (uint8_t *)malloc(len ? len : 1), out = (uint8_t *)malloc(cap);
            work = (uint8_t *)aligned_alloc(16, wbytes);
            if (fread(in, 1, len, f) != (size_t)len) _Exit(2);
            memset(&S, 0xCD, sizeof S);   // LDS holds anything at launch
            memset(work, 0xCD, wbytes);
        }
        BZE_SYNC();
        got_of[tid] = bzip2_stream(S, tid, in, len, (int)level, out, cap, work);
        BZE_SYNC();
        if (tid == 0) {
            for (int t = 1; t < HOST_T; ++t)
                if (got_of[t] != got_of[0]) {
                    fprintf(stderr, "stream %lld: thread %d returns %lld; thread 0 %lld\n", (long long)i, t, (long long)got_of[t], (long long)got_of[0]);
                    _Exit(8);
                }
            fwrite(&got_of[0], 8, 1, g);
            fwrite(&cap, 8, 1, g);
            fwrite(&wbytes, 8, 1, g);
            if (got_of[0] > cap) _Exit(4);
            if (got_of[0] > 0) fwrite(out, 1, got_of[0], g);
            free(in);
            free(out);
            free(work);
        }
    }
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    f = fopen(argv[1], "rb"), g = fopen(argv[2], "wb");
    if (!f || !g || fread(&n, 8, 1, f) != 1) return 2;
#if HOST_T == 1
    threads(0);
#else
    hw::run(threads);
#endif
    return fclose(g) ? 2 : 0;
}
