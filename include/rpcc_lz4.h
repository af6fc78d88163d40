/*
 * rpcc_lz4.h -- C ABI of librpcc_lz4.so: the LZ4 entropy back-end on the MI355X (gfx950), the device counterpart of the
 * reference's basic_compressor 'lz4' (utils/compress_utils.py:232-310, python-lz4 0.7.0 dumps / loads).  A library of its
 * own, apart from librpcc_hip.so.
 *
 * Conventions as in rpcc_seg.h: plain pointers and sizes; every pointer marked "dev" is a device pointer; kernels are
 * enqueued on the caller's hipStream_t (passed as void*) and nothing synchronises; the library allocates nothing; 0 = OK,
 * negative = error with the text in rpcc_lz4_last_error().  Argument errors return RPCC_LZ4_ERR_ARG before anything
 * touches the device.
 *
 * A stream in "dumps form" is a uint32 little-endian uncompressed size n followed by one raw LZ4 block.  The encoder's
 * parse is the build's own, pinned bit for bit: hash5 at hashLog 14 over every earlier position,
 * greedy, no backward extension.  The decoder reads any LZ4 block.
 *
 * Batches are given by descriptors in device memory: stream s reads src_len[s] bytes at the device address src_ptr[s] and
 * writes into dst[dst_off[s] .. dst_off[s] + dst_cap[s]).  Nothing outside these ranges is read or written.
 */
#ifndef RPCC_LZ4_H
#define RPCC_LZ4_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RPCC_LZ4_ABI_VERSION 1
#define RPCC_LZ4_ERR_ARG (-1)
#define RPCC_LZ4_ERR_HIP (-2)
#define RPCC_LZ4_MAX_INPUT 0x7E000000     /* bytes per stream (LZ4_MAX_INPUT_SIZE) */
#define RPCC_LZ4_MAX_STREAMS 0x7FFFFFFF   /* streams per call: the stream index is a grid dimension */

/* Per-stream results of rpcc_lz4_decode (status) and rpcc_lz4_encode (dst_len < 0). */
#define RPCC_LZ4_OK 0
#define RPCC_LZ4_E_CAPACITY (-1)   /* header size (decode) or bound (encode) larger than the stream's capacity */
#define RPCC_LZ4_E_TRUNCATED (-2)  /* header, token, length byte, literal or offset runs past the input */
#define RPCC_LZ4_E_OFFSET (-3)     /* offset 0 or beyond the bytes produced so far */
#define RPCC_LZ4_E_OVERRUN (-4)    /* literals or a match would produce more than the header's size */
#define RPCC_LZ4_E_SIZE (-5)       /* the block ends having produced fewer bytes than the header's size */

int rpcc_lz4_version(void);
const char *rpcc_lz4_last_error(void);

/* Worst-case size of one stream in dumps form: 4 + n + n/255 + 16 (0 for n < 0 or n > RPCC_LZ4_MAX_INPUT). */
size_t rpcc_lz4_bound(int64_t n);

/* Bytes of the work buffer rpcc_lz4_pack_containers takes for nstreams streams (0 for an invalid count). */
size_t rpcc_lz4_workspace_bytes(int64_t nstreams);
/* Caller's buffers: ws needs no initialisation (it may hold anything, an earlier call's contents included), nothing outside the size above
 * is touched and its contents are undefined on return; align it to 8 bytes (the tests use 256, and base + 8 once).  dst / out are written only where a stream
 * or container lands: dst[dst_off[s] .. + dst_len[s]) -- the rest of a slot, the gaps between slots and a refused stream's slot are left
 * as they are.  dst_len, status, frame_off and frame_len are written for every stream / frame. */

/* Encode nstreams streams into dumps form.  src_ptr (dev, uint64 [nstreams]) device addresses, src_len (dev, int64) their
 * lengths; stream s is written at dst + dst_off[s] (dev, int64), which must have room for dst_cap[s] (dev, int64) >=
 * rpcc_lz4_bound(src_len[s]) bytes.  dst_len (dev, int64 [nstreams]): bytes written, or RPCC_LZ4_E_CAPACITY when the length
 * is out of range or the slot too small (nothing is written then). */
int rpcc_lz4_encode(const uint64_t *src_ptr, const int64_t *src_len, int64_t nstreams, uint8_t *dst, const int64_t *dst_off,
                    const int64_t *dst_cap, int64_t *dst_len, void *stream);

/* The .rpcc containers of nframes frames of per_frame streams each (frame f owns streams f*per_frame .. +per_frame-1, in
 * container order): [int32 length | stream bytes] per stream, frames back to back in out (dev, out_cap bytes).  slots,
 * dst_off, dst_len as rpcc_lz4_encode wrote them.  frame_off, frame_len (dev, int64 [nframes]): each container's place in
 * out; frame_len is -1 for a frame with a failed stream or one that does not fit in out_cap (it is not written).
 * ws: rpcc_lz4_workspace_bytes(nframes * per_frame) bytes. */
int rpcc_lz4_pack_containers(const uint8_t *slots, const int64_t *dst_off, const int64_t *dst_len, int64_t nframes, int per_frame,
                             uint8_t *out, int64_t out_cap, int64_t *frame_off, int64_t *frame_len, void *ws, void *stream);

/* Decode nstreams dumps-form streams (src_ptr, src_len as for encode) into dst + dst_off[s], at most dst_cap[s] bytes.
 * status (dev, int32 [nstreams]): RPCC_LZ4_OK or one of RPCC_LZ4_E_*; dst_len (dev, int64): bytes produced (the header's
 * size when OK).  A header-only 4-byte stream of size 0 is accepted. */
int rpcc_lz4_decode(const uint64_t *src_ptr, const int64_t *src_len, int64_t nstreams, uint8_t *dst, const int64_t *dst_off,
                    const int64_t *dst_cap, int64_t *dst_len, int32_t *status, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* RPCC_LZ4_H */
