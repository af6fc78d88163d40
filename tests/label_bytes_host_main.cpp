// csrc/label_bytes.h built for the host and held to a byte loop: every pair of label bytes in every pair of positions of a word against every
// label, random words against random labels with random pending marks, and a whole 16-pixel lane counted label by label the way
// count_tile_row (rpcc_hip.hip) does it.  Prints "checked N bad 0"; exit status 1 if anything differs.
#include <stdint.h>
#include <stdio.h>

#include "label_bytes.h"

static uint32_t rng_state = 0x9E3779B9u;
static uint32_t rnd() {   // xorshift32
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5;
    return rng_state;
}

static uint32_t eq_loop(uint32_t w, uint32_t label) {
    uint32_t m = 0;
    for (int i = 0; i < 4; i++)
        if (((w >> (8 * i)) & 255u) == label) m |= 0x80u << (8 * i);
    return m;
}

static long long checked = 0, bad = 0;
static void check_word(uint32_t w, uint32_t label, uint32_t pending) {
    const uint32_t want = eq_loop(w, label);
    checked++;
    if (rpcc_label_eq_bytes(w, label) != want) bad++;
    uint32_t p = pending;
    const uint32_t n = rpcc_label_count_word(w, label, &p);
    if (n != (uint32_t)__builtin_popcount(want & pending) || p != (pending & ~want)) bad++;
}

// a lane's 16 pixels, the first nval of them valid: the counts per label as count_tile_row finds them
static void check_lane(const uint8_t *px, int nval) {
    uint32_t w[4] = {0, 0, 0, 0}, pend[4], got[256] = {0}, want[256] = {0};
    for (int e = 0; e < 16; e++) w[e >> 2] |= (uint32_t)px[e] << (8 * (e & 3));
    for (int e = 0; e < nval; e++) want[px[e]]++;
    for (int d = 0; d < 4; d++) pend[d] = rpcc_label_marks(nval - 4 * d);
    int steps = 0;
    while ((pend[0] | pend[1] | pend[2] | pend[3]) != 0u && steps++ < 17) {
        uint32_t p = pend[0], x = w[0];
        if (p == 0u) { p = pend[1]; x = w[1]; }
        if (p == 0u) { p = pend[2]; x = w[2]; }
        if (p == 0u) { p = pend[3]; x = w[3]; }
        const uint32_t cur = (x >> (__builtin_ffs((int)p) - 8)) & 255u;
        for (int d = 0; d < 4; d++) got[cur] += rpcc_label_count_word(w[d], cur, &pend[d]);
    }
    checked++;
    if (steps > 16) bad++;
    for (int k = 0; k < 256; k++)
        if (got[k] != want[k]) { bad++; break; }
}

int main() {
    // all 2^16 pairs of (two label bytes) x every target label x every pair of positions, the other bytes 0x00 / 0xFF / 0x01 / 0x80
    static const uint32_t fill[4] = {0x00000000u, 0xFFFFFFFFu, 0x01010101u, 0x80808080u};
    for (uint32_t a = 0; a < 256; a++)
        for (uint32_t b = 0; b < 256; b++)
            for (int i = 0; i < 4; i++)
                for (int j = 0; j < 4; j++) {
                    if (i == j) continue;
                    for (int f = 0; f < 4; f++) {
                        const uint32_t keep = ~((255u << (8 * i)) | (255u << (8 * j)));
                        const uint32_t w = (fill[f] & keep) | (a << (8 * i)) | (b << (8 * j));
                        const uint32_t labels[6] = {a, b, (a + 1) & 255u, (b - 1) & 255u, a ^ 0x80u, fill[f] & 255u};
                        for (int l = 0; l < 6; l++) check_word(w, labels[l], 0x80808080u);
                    }
                }
    for (uint32_t a = 0; a < 256; a++)      // two equal or different bytes in the low half against EVERY label
        for (uint32_t b = 0; b < 256; b++)
            for (uint32_t t = 0; t < 256; t++) check_word(a | (b << 8) | (rnd() & 0xFFFF0000u), t, 0x80808080u);
    for (int i = 0; i < 4000000; i++) {
        const uint32_t w = rnd(), t = (i & 1) ? ((w >> (8 * (rnd() & 3))) & 255u) : (rnd() & 255u);
        check_word(w, t, rnd() & 0x80808080u);
    }
    for (int n = 0; n <= 4; n++) {
        checked++;
        uint32_t want = 0;
        for (int i = 0; i < n; i++) want |= 0x80u << (8 * i);
        if (rpcc_label_marks(n) != want) bad++;
    }
    if (rpcc_label_marks(-3) != 0u || rpcc_label_marks(9) != 0x80808080u) bad++;
    for (int i = 0; i < 300000; i++) {
        uint8_t px[16];
        const int kinds = 1 + (int)(rnd() % 16u), nval = (i % 5 == 0) ? (int)(rnd() % 17u) : 16;
        uint8_t pool[16];
        for (int k = 0; k < 16; k++) pool[k] = (uint8_t)rnd();
        for (int e = 0; e < 16; e++) px[e] = (i % 7 == 0) ? (uint8_t)(e * 16 + (i & 15)) : pool[rnd() % (uint32_t)kinds];
        check_lane(px, nval);
    }
    printf("checked %lld bad %lld\n", checked, bad);
    return bad ? 1 : 0;
}
