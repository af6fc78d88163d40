/*
 * rpcc_deflate.h -- C ABI of librpcc_deflate.so: the gzip / deflate entropy back-end on the MI355X (gfx950), the device
 * counterpart of the reference's basic_compressor 'deflate' / 'gzip' (utils/compress_utils.py:232-310, gzip.compress).  A
 * library of its own, apart from librpcc_hip.so.  Any inflate reads the streams; the device decoder is librpcc_inflate.so (rpcc_inflate.h).
 *
 * Conventions as in rpcc_lz4.h: plain pointers and sizes; every pointer marked "dev" is a device pointer; kernels are
 * enqueued on the caller's hipStream_t (passed as void*) and nothing synchronises; the library allocates nothing; 0 = OK,
 * negative = error with the text in rpcc_deflate_last_error().  Argument errors return RPCC_DEFLATE_ERR_ARG before anything
 * touches the device.
 *
 * A stream is one gzip member: the 10 bytes 1f 8b 08 00 00 00 00 00 00 ff, a raw deflate body of one dynamic block (or of
 * stored blocks where that is not larger), crc32 and size.  The parse and the code lengths are the build's own, pinned bit
 * for bit: the LZ4 encoder's greedy parse with a 32768-byte window, length-limited Huffman codes.
 *
 * Batches are given by descriptors in device memory: stream s reads src_len[s] bytes at the device address src_ptr[s] and
 * writes into dst[dst_off[s] .. dst_off[s] + dst_cap[s]).  Nothing outside these ranges and the workspace is read or written.
 */
#ifndef RPCC_DEFLATE_H
#define RPCC_DEFLATE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RPCC_DEFLATE_ABI_VERSION 1
#define RPCC_DEFLATE_ERR_ARG (-1)
#define RPCC_DEFLATE_ERR_HIP (-2)
#define RPCC_DEFLATE_MAX_INPUT 0x7E000000     /* bytes per stream */
#define RPCC_DEFLATE_MAX_STREAMS 0x7FFFFFFF   /* streams per call: the stream index is a grid dimension */

/* Per-stream result of rpcc_deflate_encode (dst_len < 0). */
#define RPCC_DEFLATE_E_CAPACITY (-1)   /* length out of range, slot below the bound, or the workspace too small for the stream */

int rpcc_deflate_version(void);
const char *rpcc_deflate_last_error(void);

/* Worst-case size of one stream: 18 + n + 5 * max(1, ceil(n / 65535)) (0 for n < 0 or n > RPCC_DEFLATE_MAX_INPUT). */
size_t rpcc_deflate_bound(int64_t n);

/* Bytes of the work buffer rpcc_deflate_encode takes for nstreams streams of total_len input bytes in all (an upper bound of
 * the sum of src_len is enough); 0 for an invalid count or total. */
size_t rpcc_deflate_workspace_bytes(int64_t nstreams, int64_t total_len);
/* Caller's buffers: ws needs no initialisation (it may hold anything, an earlier call's contents under other arguments included), nothing
 * outside the size above is touched and its contents are undefined on return; align it to 8 bytes (the tests use 256, and base + 8 once).  dst is written
 * only where a member lands: dst[dst_off[s] .. + dst_len[s]) -- the rest of a slot, the gaps between slots and a refused stream's slot
 * are left as they are; dst_len is written for every stream. */

/* Encode nstreams streams as gzip members.  src_ptr (dev, uint64 [nstreams]) device addresses, src_len (dev, int64) their
 * lengths; stream s is written at dst + dst_off[s] (dev, int64), which must have room for dst_cap[s] (dev, int64) >=
 * rpcc_deflate_bound(src_len[s]) bytes.  dst_len (dev, int64 [nstreams]): bytes written, or RPCC_DEFLATE_E_CAPACITY when the
 * length is out of range, the slot too small or the sum of the lengths above total_len (nothing is written to the slot then).
 * ws (dev): rpcc_deflate_workspace_bytes(nstreams, total_len) bytes, 8-byte aligned. */
int rpcc_deflate_encode(const uint64_t *src_ptr, const int64_t *src_len, int64_t nstreams, int64_t total_len, uint8_t *dst,
                        const int64_t *dst_off, const int64_t *dst_cap, int64_t *dst_len, void *ws, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* RPCC_DEFLATE_H */
