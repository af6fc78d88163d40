/*
 * rpcc_bzip2.h -- C ABI of librpcc_bzip2.so: the bzip2 encoder on the MI355X (gfx950), the device counterpart of the reference's
 * basic_compressor 'bzip2' (utils/compress_utils.py:232-310, bz2.compress).  A library of its own, apart from librpcc_hip.so.  Any
 * bunzip2 reads the streams; the device decoder is librpcc_bunzip2.so (rpcc_bunzip2.h).
 *
 * Conventions as in rpcc_deflate.h: plain pointers and sizes; every pointer marked "dev" is a device pointer; kernels are enqueued on the
 * caller's hipStream_t (passed as void*) and nothing synchronises; the library allocates nothing; 0 = OK, negative = error with the text
 * in rpcc_bzip2_last_error().  Argument errors return RPCC_BZIP2_ERR_ARG before anything touches the device.
 *
 * A stream is one bzip2 stream: "BZh" and the level digit, the blocks (100000 * level - 19 bytes after RLE1 at most), the end magic and
 * the combined CRC.  The bytes are the build's own, pinned bit for bit (tests/bzip2_ref.py): the format's RLE1,
 * rotation sort and move-to-front, the build's rules for the block cut, the tables and their length-limited codes.
 *
 * Batches are given by descriptors in device memory: stream s reads src_len[s] bytes at the device address src_ptr[s] and writes into
 * dst[dst_off[s] .. dst_off[s] + dst_cap[s]).  Nothing outside these ranges and the workspace is read or written.
 */
#ifndef RPCC_BZIP2_H
#define RPCC_BZIP2_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RPCC_BZIP2_ABI_VERSION 1
#define RPCC_BZIP2_ERR_ARG (-1)
#define RPCC_BZIP2_ERR_HIP (-2)
#define RPCC_BZIP2_MAX_INPUT 0x7E000000     /* bytes per stream */
#define RPCC_BZIP2_MAX_STREAMS 0x7FFFFFFF   /* streams per call: the stream index is a grid dimension */

/* Per-stream result of rpcc_bzip2_encode (dst_len < 0). */
#define RPCC_BZIP2_E_CAPACITY (-1)   /* length out of range, slot below the bound, or the workspace too small for the stream */

int rpcc_bzip2_version(void);
const char *rpcc_bzip2_last_error(void);

/* Worst-case size of one stream of n bytes at level 1..9, from the specification: m = n + n / 4 bytes after RLE1 in
 * nb = max(1, ceil(m / (100000 * level - 23))) blocks; 14 + nb * 6450 + ceil((17 * (m + nb) + 6 * ((m + nb) / 50 + nb)) / 8).
 * 0 for n < 0, n > RPCC_BZIP2_MAX_INPUT or a level outside 1..9. */
size_t rpcc_bzip2_bound(int64_t n, int level);

/* Bytes of the work buffer rpcc_bzip2_encode takes for nstreams streams of total_len input bytes in all (an upper bound of the sum of
 * src_len is enough): 256-aligned 8 * nstreams, then 23 * (total_len + total_len / 4) + 944 * nstreams; 0 for an invalid count, total or level. */
size_t rpcc_bzip2_workspace_bytes(int64_t nstreams, int64_t total_len, int level);
/* Caller's buffers: ws needs no initialisation (it may hold anything, an earlier call's contents under other arguments included), nothing
 * outside the size above is touched and its contents are undefined on return; align it to 16 bytes.  dst is written only where a stream
 * lands: dst[dst_off[s] .. + dst_len[s]) -- the rest of a slot, the gaps between slots and a refused stream's slot are left as they are;
 * dst_len is written for every stream. */

/* Encode nstreams streams as bzip2 streams of this level.  src_ptr (dev, uint64 [nstreams]) device addresses, src_len (dev, int64) their
 * lengths; stream s is written at dst + dst_off[s] (dev, int64), which must have room for dst_cap[s] (dev, int64) >=
 * rpcc_bzip2_bound(src_len[s], level) bytes.  dst_len (dev, int64 [nstreams]): bytes written, or RPCC_BZIP2_E_CAPACITY when the length is
 * out of range, the slot too small or the sum of the lengths above total_len (nothing is written to the slot then).  ws (dev): rpcc_bzip2_workspace_bytes(nstreams, total_len, level) bytes, 16-byte aligned. */
int rpcc_bzip2_encode(const uint64_t *src_ptr, const int64_t *src_len, int64_t nstreams, int64_t total_len, int level, uint8_t *dst,
                      const int64_t *dst_off, const int64_t *dst_cap, int64_t *dst_len, void *ws, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* RPCC_BZIP2_H */
