// The decoder of csrc_bunzip2/bunzip2_core.h as a host program (tests/test_bunzip2_core_host.py): the same text the gfx950 kernel is
// compiled from.  By default the wave has one lane, so the statuses and bytes are the kernel's but for what the lanes do in parallel; with
// -DHOST_LANES=64 (the test reads BZ_WAVE from bunzip2_kernels.hip) the lanes are threads of tests/host_wave.h, which is where barriers,
// ballots, shuffles, the LDS atomics and the claims of BZ_UNI are run, under a thread sanitizer too.  Every lane must return the same
// status and counts.
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
#ifndef HOST_LANES
#define HOST_LANES 1
#endif
#define BZ_WAVE HOST_LANES
#if HOST_LANES == 1
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
#define GROUP_SYNC() ((void)0)
#else
#define HW_T HOST_LANES
#define HW_WAVE HOST_LANES
#include "host_wave.h"
#define BZ_SYNC() hw::sync(HW_AT)
#define BZ_UNI(x) hw::uni((int)(x), HW_AT)
#define BZ_BALLOT(p) hw::ballot((p), HW_AT)
#define BZ_SHFL_XOR(v, m) hw::shfl_xor((v), (m), HW_AT)
#define BZ_SHFL_UP(v, d) hw::shfl_up((v), (d), HW_AT)
#define BZ_READLANE(v, l) hw::readlane((int)(v), (l), HW_AT)
#define BZ_LDS_ADD(p, v) hw::lds_add((p), (v))
#define BZ_LDS_FETCH_ADD(p, v) hw::lds_fetch_add((p), (v))
#define GROUP_SYNC() hw::sync(HW_AT)
#endif
#include "bunzip2_core.h"

static FILE *f, *g;
static int64_t n, len, cap, blk, wbytes, status_of[HOST_LANES], produced_of[HOST_LANES], used_of[HOST_LANES];
static uint8_t *in, *out, *work;
static BzShared S;

// every lane runs the streams in turn; lane 0 reads, allocates and writes between two barriers
static void lanes(int lane) {
    for (int64_t i = 0; i < n; ++i) {
        if (lane == 0) {
            if (fread(&len, 8, 1, f) != 1 || fread(&cap, 8, 1, f) != 1 || fread(&blk, 8, 1, f) != 1) _Exit(2);
            wbytes = bz_work_layout(blk).bytes;
            if (bz_work_block(wbytes) != blk) _Exit(3);      // the layout and its inverse are one statement
            in = (uint8_t *)malloc(len ? len : 1), out = (uint8_t *)malloc(cap > 0 ? cap : 1), work = (uint8_t *)malloc(wbytes ? wbytes : 4);
            if (fread(in, 1, len, f) != (size_t)len) _Exit(2);
            memset(&S, 0xCD, sizeof S);   // LDS holds anything at launch
            memset(work, 0xCD, wbytes ? wbytes : 4);
        }
        GROUP_SYNC();
        int64_t produced = -1, used = -1;
        status_of[lane] = bunzip2_stream(S, lane, in, len, out, cap, work, wbytes, produced, used);
        produced_of[lane] = produced;
        used_of[lane] = used;
        GROUP_SYNC();
        if (lane == 0) {
            for (int l = 1; l < HOST_LANES; ++l)
                if (status_of[l] != status_of[0] || produced_of[l] != produced_of[0] || used_of[l] != used_of[0]) {
                    fprintf(stderr, "stream %lld: lane %d returns %lld, %lld, %lld; lane 0 %lld, %lld, %lld\n", (long long)i, l, (long long)status_of[l],
                            (long long)produced_of[l], (long long)used_of[l], (long long)status_of[0], (long long)produced_of[0], (long long)used_of[0]);
                    _Exit(8);
                }
            fwrite(&status_of[0], 8, 1, g);
            fwrite(&produced_of[0], 8, 1, g);
            fwrite(&used_of[0], 8, 1, g);
            if (status_of[0] == RPCC_BUNZIP2_OK) fwrite(out, 1, produced_of[0], g);
            if (status_of[0] == RPCC_BUNZIP2_E_OVERRUN) fwrite(out, 1, cap, g);
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
#if HOST_LANES == 1
    lanes(0);
#else
    hw::run(lanes);
#endif
    return fclose(g) ? 2 : 0;
}
