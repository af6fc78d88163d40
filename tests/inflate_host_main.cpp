// The decoder of csrc_inflate/inflate_core.h as a host program (tests/test_inflate_core_host.py): the same text the gfx950 kernel is
// compiled from.  By default the wave has one lane, so the statuses and bytes are the kernel's but for what the lanes do in parallel; with
// -DHOST_LANES=64 (the test reads INF_WAVE from inflate_kernels.hip) the lanes are threads of tests/host_wave.h, which is where barriers,
// ballots, shuffles and the claims of INF_UNI are run, under a thread sanitizer too.  Every lane must return the same status and count.
// Input file: int64 count, then per stream int64 length, int64 capacity, bytes.  Output file: per stream int64 status, int64 produced, bytes if OK.
// Source and destination are heap blocks of exactly the stated sizes, so a sanitizer build (-fsanitize=address,undefined) sees any overrun.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "rpcc_inflate.h"

#define INF_FN static inline
#define INF_CONST static const
#ifndef HOST_LANES
#define HOST_LANES 1
#endif
#define INF_WAVE HOST_LANES
#if HOST_LANES == 1
#define INF_SYNC() ((void)0)
#define INF_UNI(x) ((int)(x))
#define INF_BALLOT(p) ((p) ? 1ull : 0ull)
#define INF_SHFL_XOR(v, m) (v)
#define GROUP_SYNC() ((void)0)
#else
#define HW_T HOST_LANES
#define HW_WAVE HOST_LANES
#include "host_wave.h"
#define INF_SYNC() hw::sync(HW_AT)
#define INF_UNI(x) hw::uni((int)(x), HW_AT)
#define INF_BALLOT(p) hw::ballot((p), HW_AT)
#define INF_SHFL_XOR(v, m) hw::shfl_xor((v), (m), HW_AT)
#define GROUP_SYNC() hw::sync(HW_AT)
#endif
static inline uint32_t brev32(uint32_t x) {
    uint32_t r = 0;
    for (int i = 0; i < 32; ++i) r |= ((x >> i) & 1u) << (31 - i);
    return r;
}
#define INF_BREV(x) brev32(x)
#include "inflate_core.h"

static FILE *f, *g;
static int64_t n, len, cap, status_of[HOST_LANES], produced_of[HOST_LANES];
static uint8_t *in, *out;
static InfShared S;

// every lane runs the streams in turn; lane 0 reads, allocates and writes between two barriers
static void lanes(int lane) {
    for (int64_t i = 0; i < n; ++i) {
        if (lane == 0) {
            if (fread(&len, 8, 1, f) != 1 || fread(&cap, 8, 1, f) != 1) _Exit(2);
            in = (uint8_t *)malloc(len ? len : 1), out = (uint8_t *)malloc(cap > 0 ? cap : 1);
            if (fread(in, 1, len, f) != (size_t)len) _Exit(2);
            memset(&S, 0xCD, sizeof S);   // LDS holds anything at launch
        }
        GROUP_SYNC();
        int64_t produced = -1;
        status_of[lane] = inflate_stream(S, lane, in, len, out, cap, produced);
        produced_of[lane] = produced;
        GROUP_SYNC();
        if (lane == 0) {
            for (int l = 1; l < HOST_LANES; ++l)
                if (status_of[l] != status_of[0] || produced_of[l] != produced_of[0]) {
                    fprintf(stderr, "stream %lld: lane %d returns %lld, %lld; lane 0 %lld, %lld\n", (long long)i, l, (long long)status_of[l],
                            (long long)produced_of[l], (long long)status_of[0], (long long)produced_of[0]);
                    _Exit(8);
                }
            fwrite(&status_of[0], 8, 1, g);
            fwrite(&produced_of[0], 8, 1, g);
            if (status_of[0] == 0) fwrite(out, 1, produced_of[0], g);
            free(in);
            free(out);
        }
    }
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    f = fopen(argv[1], "rb"), g = fopen(argv[2], "wb");
    if (!f || !g || fread(&n, 8, 1, f) != 1) return 2;
#if HOST_LANES == 1
    lanes(0);
#else
    hw::run(lanes);
#endif
    return fclose(g) ? 2 : 0;
}
