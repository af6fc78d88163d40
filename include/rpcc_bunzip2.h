/*
 * rpcc_bunzip2.h -- C ABI of librpcc_bunzip2.so: the bzip2 decoder on the MI355X (gfx950), the device counterpart of bz2.decompress
 * for basic_compressor 'bzip2' (the default of cfgs/compressor.yaml).  A library of its own, apart from librpcc_hip.so and from the
 * other entropy libraries.
 *
 * Conventions as in rpcc_inflate.h: plain pointers and sizes; every pointer marked "dev" is a device pointer; kernels are
 * enqueued on the caller's hipStream_t (passed as void*) and nothing synchronises; the library allocates nothing; 0 = OK,
 * negative = error with the text in rpcc_bunzip2_last_error().  Argument errors return RPCC_BUNZIP2_ERR_ARG before anything
 * touches the device.
 *
 * A stream is one bzip2 stream: "BZh", a level '1'..'9', any number of blocks (none: bz2.compress(b"")), the end-of-stream
 * magic and the combined CRC, padded to a byte; then nothing.  What is accepted is what libbz2 1.0.8 accepts, with the same
 * bytes: 2 to 6 coding tables; 1 to 32767 selectors, of which those past 18002 are read and dropped; code lengths 1 to 20, not
 * checked for being a prefix code -- a symbol is what libbz2's limit / base / perm rule reads, bit by bit from the shortest
 * length, 20 bits at most; a symbol map with no byte in use is refused; a run may not pass 2^21 in its binary weight nor the
 * block 100000 * level bytes; the origin pointer must lie inside the block (and below 100000 * level + 11 where it is read);
 * the first run-length stage starts anew in every block, and a block that ends on four equal bytes with no count behind them is
 * refused (libbz2 reads the count from beyond the block and then calls the block corrupt).  A block with the randomised bit is
 * refused (libbz2 still decodes those), and so is any byte after the stream, a second stream included (bz2.decompress
 * concatenates streams and ignores other trailing bytes): nothing this project writes has either.
 *
 * Batches are given by descriptors in device memory: stream s reads src_len[s] bytes at the device address src_ptr[s], writes
 * into dst[dst_off[s] .. dst_off[s] + dst_cap[s]) and uses work[work_off[s] .. work_off[s] + work_cap[s]) for its blocks.  No
 * stream, however malformed, makes the decoder read outside its source or write outside these two slots.
 *
 * The work slot.  rpcc_bunzip2_stream_work_bytes(m) is what a stream needs whose blocks hold up to m bytes (counted before the
 * inverse of the first run-length stage, as bzip2 counts them); the kernel carves the slot with the same layout function.  A
 * block of a stream of level L that decodes to at most dst_cap bytes holds at most
 *     min(100000 * L, 5 * dst_cap / 4 + 8)
 * bytes: each of them gives at least one byte of output but a count byte, and at most every fifth is a count byte.  work +
 * work_off[s] must be a multiple of 4.  A block longer than the slot holds ends the stream with RPCC_BUNZIP2_E_WORK.
 */
#ifndef RPCC_BUNZIP2_H
#define RPCC_BUNZIP2_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RPCC_BUNZIP2_ABI_VERSION 1
#define RPCC_BUNZIP2_ERR_ARG (-1)
#define RPCC_BUNZIP2_ERR_HIP (-2)
#define RPCC_BUNZIP2_MAX_STREAMS 0x7FFFFFFF   /* streams per call: the stream index is a grid dimension */
#define RPCC_BUNZIP2_MAX_BLOCK 900000         /* the longest block of any stream: level 9 */

/* Per-stream status: the first check that fails, in stream order.  (-1 is not used: the numbers line up with RPCC_INFLATE_E_*.) */
#define RPCC_BUNZIP2_OK 0
#define RPCC_BUNZIP2_E_TRUNCATED (-2)   /* any read past src_len */
#define RPCC_BUNZIP2_E_HEADER (-3)      /* stream magic or level */
#define RPCC_BUNZIP2_E_MAGIC (-4)       /* the 48 bits are neither a block magic nor the end-of-stream magic */
#define RPCC_BUNZIP2_E_RANDOMISED (-5)  /* the obsolete randomised bit is set */
#define RPCC_BUNZIP2_E_TABLE (-6)       /* symbol map, group count, selector or code-length rules */
#define RPCC_BUNZIP2_E_SYMBOL (-7)      /* bits that match no code, more groups than selectors, a run or block past 100000 * level */
#define RPCC_BUNZIP2_E_ORIGPTR (-8)     /* origin pointer outside the block */
#define RPCC_BUNZIP2_E_OVERRUN (-9)     /* the stream is sound but decodes to more than dst_cap: dst_len is its size */
#define RPCC_BUNZIP2_E_CRC (-10)        /* block CRC or combined CRC */
#define RPCC_BUNZIP2_E_WORK (-11)       /* a block is longer than the work slot holds (or the slot is not 4-byte aligned) */
#define RPCC_BUNZIP2_E_TRAILING (-12)   /* any byte after the stream */
#define RPCC_BUNZIP2_E_RLE (-13)        /* a block ends on four equal bytes with no count byte */

int rpcc_bunzip2_version(void);
const char *rpcc_bunzip2_last_error(void);

/* Bytes of work slot for a stream whose blocks hold up to nblock_max bytes (0 .. RPCC_BUNZIP2_MAX_BLOCK; more counts as
 * RPCC_BUNZIP2_MAX_BLOCK).  Monotone; a multiple of 4 is not promised -- round the slots' offsets up.  Negative: RPCC_BUNZIP2_ERR_ARG. */
int64_t rpcc_bunzip2_stream_work_bytes(int64_t nblock_max);

/* Decode nstreams bzip2 streams.  Stream s reads src_len[s] bytes at device address src_ptr[s] (any byte alignment), writes at
 * dst + dst_off[s] (any alignment) at most dst_cap[s] bytes, and uses work + work_off[s], work_cap[s] bytes.  status (dev, int32
 * [nstreams]) RPCC_BUNZIP2_OK or E_*; dst_len (dev, int64 [nstreams]); src_used (dev, int64 [nstreams]) the input bytes read: on OK
 * the stream's length with its padding to a byte.
 * On OK exactly dst[dst_off[s] .. + dst_len[s]) is written.  RPCC_BUNZIP2_E_OVERRUN is a complete answer: the decoder stores
 * nothing past dst_cap[s], runs every remaining check, and dst_len[s] is the size the stream decodes to, so one more call with that
 * capacity decodes it.  On any other error dst_len[s] is the size of the blocks decoded before the failure: the slot's bytes are
 * undefined.  The work slot's contents before the call do not matter and are undefined after it.  dst_len, src_used and status
 * are written for every stream; the gaps between slots are left as they are.  nstreams == 0 returns 0 and launches nothing. */
int rpcc_bunzip2_decode(const uint64_t *src_ptr, const int64_t *src_len, int64_t nstreams, uint8_t *dst, const int64_t *dst_off,
                        const int64_t *dst_cap, uint8_t *work, const int64_t *work_off, const int64_t *work_cap, int64_t *dst_len,
                        int64_t *src_used, int32_t *status, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* RPCC_BUNZIP2_H */
