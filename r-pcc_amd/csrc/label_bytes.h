/* label_bytes.h -- four byte labels in a word, compared at once: what count_scan_kernel (rpcc_hip.hip) counts a lane's 16 pixels with.
 * Plain C (also compiled as C++ and as HIP device code): the same text is built into librpcc_hip.so and into tests/label_bytes_host_main.cpp,
 * which holds it to a byte loop over every pair of bytes against every label and over random words. */
#ifndef RPCC_LABEL_BYTES_H
#define RPCC_LABEL_BYTES_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RPCC_LB_FN __host__ __device__ static inline __attribute__((always_inline))
#else
#define RPCC_LB_FN static inline
#endif

/* 0x80 in every byte of w that equals label (0 .. 255), 0 in the others.  With y = w ^ (label in every byte) a byte of y is zero exactly
 * where the labels agree; (y & 0x7F) + 0x7F sets bit 7 of a byte unless its low seven bits are zero and never carries into the next byte
 * (at most 0xFE), | y brings in the byte's own bit 7: bit 7 stays clear for a zero byte alone.  Exact for every byte value -- unlike
 * (y - 0x01010101) & ~y & 0x80808080, whose borrow marks a 0x01 above a zero byte. */
RPCC_LB_FN uint32_t rpcc_label_eq_bytes(uint32_t w, uint32_t label) {
    const uint32_t y = w ^ (label * 0x01010101u);
    return ~(((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y) & 0x80808080u;
}

/* How many of the word's bytes that `pending` marks (0x80 per byte) equal label; those bytes' marks are taken out of *pending. */
RPCC_LB_FN uint32_t rpcc_label_count_word(uint32_t w, uint32_t label, uint32_t *pending) {
    const uint32_t eq = rpcc_label_eq_bytes(w, label) & *pending;
    *pending ^= eq;
    return (uint32_t)__builtin_popcount(eq); /* 0 .. 4 */
}

/* The marks of the first n (0 .. 4) bytes of a word. */
RPCC_LB_FN uint32_t rpcc_label_marks(int n) { return n >= 4 ? 0x80808080u : n <= 0 ? 0u : (0x80808080u & ((1u << (8 * n)) - 1u)); }

#endif
