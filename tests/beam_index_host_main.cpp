// rpcc_beam_index_build (csrc/beam_index.h) as a host program (tests/test_beam_table_abi.py): the same text librpcc_hip.so is built from.
// Runs the builder over H = 1 .. 128 with sorted, descending, shuffled, constant and duplicated tables into heap blocks of exactly
// RPCC_BEAM_INDEX_BYTES(H) bytes, so a sanitizer build (-fsanitize=address,undefined) sees any overrun, and checks every index against the
// definition: the row-order copy, an ascending permutation of the table, the fp32 midpoints, the lowest row for equal entries.
// Output file (argv[1]): per table int64 H, then the index bytes -- compared with numpy by the test.  Exit status 0 = all checks held.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "beam_index.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}

static int check(const double *va, int H, const char *idx) {
    const double *a = (const double *)idx, *s = (const double *)(idx + (size_t)H * 8);
    const float *mid = (const float *)(idx + (size_t)H * 16);
    const int32_t *row = (const int32_t *)(idx + (size_t)H * 20);
    if (memcmp(a, va, (size_t)H * 8) != 0) return 1;
    for (int k = 0; k < H; k++) {
        if (row[k] < 0 || row[k] >= H || va[row[k]] != s[k]) return 2;
        for (int h = 0; h < row[k]; h++)
            if (va[h] == s[k]) return 3;   // not the lowest row of an equal entry
        if (k + 1 < H && (s[k] > s[k + 1] || mid[k] != (float)(s[k] * 0.5 + s[k + 1] * 0.5))) return 4;
    }
    if (!std::isinf(mid[H - 1]) || mid[H - 1] < 0) return 5;
    double sum_a = 0, sum_s = 0;   // a permutation: same multiset (checked through the sorted order of both)
    for (int h = 0; h < H; h++) { sum_a += va[h]; sum_s += s[h]; }
    if (std::fabs(sum_a - sum_s) > 1e-9 * (1 + std::fabs(sum_a))) return 6;
    return 0;
}

int main(int argc, char **argv) {
    FILE *out = argc > 1 ? fopen(argv[1], "wb") : nullptr;
    int tables = 0;
    for (int H = 1; H <= RPCC_BEAM_MAX_H; H++) {
        for (int kind = 0; kind < 5; kind++) {
            double *va = (double *)malloc((size_t)H * 8);
            char *idx = (char *)malloc(RPCC_BEAM_INDEX_BYTES(H));
            for (int h = 0; h < H; h++) {
                const double v = -0.43 + 0.0073 * h + 1e-4 * (rnd() % 64);
                va[h] = kind == 0 ? -0.43 + 0.0073 * h : kind == 1 ? 0.3 - 0.0073 * h : kind == 2 ? v : kind == 3 ? 0.125 : 0.01 * (int)(rnd() % (1 + H / 3));
            }
            if (kind == 2)
                for (int h = H - 1; h > 0; h--) { const int j = (int)(rnd() % (uint32_t)(h + 1)); const double t = va[h]; va[h] = va[j]; va[j] = t; }
            if (kind == 4 && H > 2) va[H - 1] = -0.0, va[0] = 0.0;   // (equal to each other)
            memset(idx, 0xCD, RPCC_BEAM_INDEX_BYTES(H));
            if (rpcc_beam_index_build_impl(va, H, idx) != 0) { fprintf(stderr, "H=%d kind=%d: refused\n", H, kind); return 1; }
            const int bad = check(va, H, idx);
            if (bad) { fprintf(stderr, "H=%d kind=%d: check %d failed\n", H, kind, bad); return 1; }
            if (out) {
                const int64_t h64 = H;
                fwrite(&h64, 8, 1, out);
                fwrite(idx, 1, RPCC_BEAM_INDEX_BYTES(H), out);
            }
            tables++;
            free(va);
            free(idx);
        }
    }
    // the refusals leave the output alone
    double bad3[3] = {0.1, NAN, 0.2};
    char buf[RPCC_BEAM_INDEX_BYTES(3)];
    memset(buf, 0x5A, sizeof(buf));
    int refused = rpcc_beam_index_build_impl(bad3, 3, buf) == -1;
    bad3[1] = -INFINITY;
    refused += rpcc_beam_index_build_impl(bad3, 3, buf) == -1;
    bad3[1] = 0.15;
    refused += rpcc_beam_index_build_impl(bad3, 0, buf) == -1;
    refused += rpcc_beam_index_build_impl(bad3, RPCC_BEAM_MAX_H + 1, buf) == -1;
    refused += rpcc_beam_index_build_impl(nullptr, 3, buf) == -1;
    refused += rpcc_beam_index_build_impl(bad3, 3, nullptr) == -1;
    for (size_t i = 0; i < sizeof(buf); i++)
        if (buf[i] != 0x5A) { fprintf(stderr, "a refused call wrote its output\n"); return 1; }
    if (refused != 6) { fprintf(stderr, "%d of 6 bad calls refused\n", refused); return 1; }
    if (out) fclose(out);
    printf("%d tables OK\n", tables);
    return 0;
}
