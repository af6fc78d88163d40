/*
 * rpcc_inflate.h -- C ABI of librpcc_inflate.so: the gzip / deflate decoder on the MI355X (gfx950), the device counterpart of
 * gzip.decompress for basic_compressor 'deflate' / 'gzip' (rpcc_deflate.h is the encoder).  A library of its own, apart from
 * librpcc_hip.so and from librpcc_deflate.so.
 *
 * Conventions as in rpcc_lz4.h: plain pointers and sizes; every pointer marked "dev" is a device pointer; kernels are
 * enqueued on the caller's hipStream_t (passed as void*) and nothing synchronises; the library allocates nothing; 0 = OK,
 * negative = error with the text in rpcc_inflate_last_error().  Argument errors return RPCC_INFLATE_ERR_ARG before anything
 * touches the device.
 *
 * A stream is one gzip member (RFC 1952), then nothing or only zero bytes; an empty stream decodes to nothing.  The header is
 * read as Python's gzip reads it: magic 1f 8b and method 8; FEXTRA skipped by its length, FNAME and FCOMMENT to their zero
 * byte, FHCRC's two bytes unchecked; FTEXT, the reserved flag bits, mtime, XFL and OS ignored.  The body is any raw deflate
 * stream (RFC 1951): stored, fixed and dynamic blocks, distances up to 32768, lengths up to 258, overlapping copies.  Code
 * lengths are accepted by zlib's rules: an over-subscribed code is an error; an incomplete one is an error for the
 * code-length code, and for the literal/length and distance codes unless its only code has length 1 (no distance code at all
 * is fine until a distance is needed); symbol 256 must have a code; HLIT > 286 or HDIST > 30 is an error.  After the last
 * block, on a byte boundary, CRC-32 and ISIZE are checked against the output.
 *
 * A second member after the first is refused (RPCC_INFLATE_E_TRAILING).  gzip.decompress would concatenate it; nothing this
 * project writes has one.
 *
 * Batches are given by descriptors in device memory: stream s reads src_len[s] bytes at the device address src_ptr[s] and
 * writes into dst[dst_off[s] .. dst_off[s] + dst_cap[s]).  No stream, however malformed, makes the decoder read or write
 * outside these ranges.
 */
#ifndef RPCC_INFLATE_H
#define RPCC_INFLATE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RPCC_INFLATE_ABI_VERSION 1
#define RPCC_INFLATE_ERR_ARG (-1)
#define RPCC_INFLATE_ERR_HIP (-2)
#define RPCC_INFLATE_MAX_STREAMS 0x7FFFFFFF   /* streams per call: the stream index is a grid dimension */

/* Per-stream status: the first check that fails, in stream order.  (-1 is not used: the numbers line up with RPCC_LZ4_E_*.) */
#define RPCC_INFLATE_OK 0
#define RPCC_INFLATE_E_TRUNCATED (-2)  /* any read past src_len: header, bits, stored bytes or trailer */
#define RPCC_INFLATE_E_HEADER (-3)     /* magic or method */
#define RPCC_INFLATE_E_BTYPE (-4)      /* block type 3 */
#define RPCC_INFLATE_E_STORED (-5)     /* LEN != ~NLEN */
#define RPCC_INFLATE_E_TABLE (-6)      /* a table rule above, a repeat with nothing before it, or a repeat past HLIT + HDIST */
#define RPCC_INFLATE_E_SYMBOL (-7)     /* bits that match no code, literal/length symbol 286 or 287, distance symbol 30 or 31 */
#define RPCC_INFLATE_E_OFFSET (-8)     /* distance beyond the bytes produced */
#define RPCC_INFLATE_E_OVERRUN (-9)    /* the output would pass dst_cap; nothing is written past it */
#define RPCC_INFLATE_E_CRC (-10)       /* CRC-32 mismatch */
#define RPCC_INFLATE_E_SIZE (-11)      /* ISIZE mismatch */
#define RPCC_INFLATE_E_TRAILING (-12)  /* a nonzero byte after the trailer (a second member included) */

int rpcc_inflate_version(void);
const char *rpcc_inflate_last_error(void);

/* Decode nstreams gzip members.  Stream s reads src_len[s] bytes at device address src_ptr[s] (any byte alignment) and writes
 * at dst + dst_off[s] (any alignment), at most dst_cap[s] bytes.  status (dev, int32 [nstreams]) RPCC_INFLATE_OK or E_*;
 * dst_len (dev, int64 [nstreams]) bytes produced.  No work buffer: the tables live in LDS.
 * On OK exactly dst[dst_off[s] .. + dst_len[s]) is written.  On an error dst_len[s] is the count produced so far: those bytes of the
 * slot are undefined, the rest of the slot is untouched.  dst_len and status are written for every stream; the gaps between slots
 * are left as they are.  nstreams == 0 returns 0 and launches nothing. */
int rpcc_inflate_decode(const uint64_t *src_ptr, const int64_t *src_len, int64_t nstreams, uint8_t *dst, const int64_t *dst_off,
                        const int64_t *dst_cap, int64_t *dst_len, int32_t *status, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* RPCC_INFLATE_H */
