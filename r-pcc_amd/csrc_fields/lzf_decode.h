// lzf_decode.h -- the liblzf stream of a .pcd file's `DATA binary_compressed` body, decoded on the host.  Plain C,
// bounds-checked; rpcc_lzf.c exports it from librpcc_host.so and tests/fields_host_main.cpp compiles it under sanitizers.
//
// A control byte c < 32 is followed by c + 1 literals.  Otherwise len = c >> 5, grown by the next byte when it is 7, the distance is
// ((c & 31) << 8 | next byte) + 1, and len + 2 bytes are copied from `distance` back, one byte at a time, so that overlaps repeat.
#ifndef RPCC_LZF_DECODE_H
#define RPCC_LZF_DECODE_H

#include <stddef.h>
#include <stdint.h>

#define LZF_OK 0
#define LZF_E_TRUNCATED 1   /* the input ends inside a literal run or a match */
#define LZF_E_DISTANCE 2    /* a match starts before the first output byte */
#define LZF_E_OVERFLOW 3    /* the output would pass dst_bytes */

/* src[0 .. src_bytes) -> dst[0 .. dst_bytes); *out_bytes: the bytes written (also when a status is returned: what stood before the
 * fault).  Nothing outside the two ranges is touched. */
static inline int lzf_decode(const uint8_t *src, size_t src_bytes, uint8_t *dst, size_t dst_bytes, size_t *out_bytes) {
    size_t ip = 0, op = 0;
    int rc = LZF_OK;
    while (ip < src_bytes) {
        const unsigned c = src[ip++];
        if (c < 32) {
            const size_t run = (size_t)c + 1;
            if (run > src_bytes - ip) { rc = LZF_E_TRUNCATED; break; }
            if (run > dst_bytes - op) { rc = LZF_E_OVERFLOW; break; }
            for (size_t k = 0; k < run; ++k) dst[op++] = src[ip++];
        } else {
            size_t len = c >> 5;
            if (len == 7) {
                if (ip >= src_bytes) { rc = LZF_E_TRUNCATED; break; }
                len += src[ip++];
            }
            if (ip >= src_bytes) { rc = LZF_E_TRUNCATED; break; }
            const size_t distance = (((size_t)c & 31) << 8 | src[ip++]) + 1;
            len += 2;
            if (distance > op) { rc = LZF_E_DISTANCE; break; }
            if (len > dst_bytes - op) { rc = LZF_E_OVERFLOW; break; }
            for (size_t k = 0; k < len; ++k, ++op) dst[op] = dst[op - distance];
        }
    }
    if (out_bytes) *out_bytes = op;
    return rc;
}

#endif /* RPCC_LZF_DECODE_H */
