/*
 * rpcc_rans.h -- C ABI of librpcc_rans.so: the chunk-parallel rANS entropy back-end on the MI355X (gfx950), basic_compressor
 * 'rans'.  A library of its own, apart from librpcc_hip.so.  The stream format (version 1, and version 2 which puts a delta
 * filter in front of the same coder) is the build's own -- DESIGN.md section 19 has it byte for byte, tests/rans_ref.py and
 * tests/rans_filter_ref.py restate it in Python -- and the reference project cannot read it: an
 * order-0 rANS coder over chunks of 2^chunk_log2 bytes, 64 interleaved states per chunk (one wavefront codes one chunk in
 * lockstep), one frequency table per byte plane (byte i of a stream is in plane i mod width) and a directory of chunk
 * lengths, so that every chunk of every stream decodes on its own.
 *
 * Conventions as in rpcc_lz4.h: plain pointers and sizes; every pointer marked "dev" is a device pointer; kernels are
 * enqueued on the caller's hipStream_t (passed as void*) and nothing synchronises; the library allocates nothing; 0 = OK,
 * negative = error with the text in rpcc_rans_last_error().  Argument errors return RPCC_RANS_ERR_ARG before anything
 * touches the device.
 *
 * Batches are given by descriptors in device memory: stream s reads src_len[s] bytes at the device address src_ptr[s] and
 * writes into dst[dst_off[s] .. dst_off[s] + dst_cap[s]).  Nothing outside these ranges is read or written.
 */
#ifndef RPCC_RANS_H
#define RPCC_RANS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RPCC_RANS_ABI_VERSION 1
#define RPCC_RANS_ERR_ARG (-1)
#define RPCC_RANS_ERR_HIP (-2)
#define RPCC_RANS_MAX_INPUT 0x7E000000     /* bytes per stream */
#define RPCC_RANS_MAX_STREAMS 0x00FFFFFF   /* streams per call */
#define RPCC_RANS_DEFAULT_CHUNK_LOG2 15    /* 32 KiB chunks; 8 .. 16 are valid */

/* The per-stream width word of rpcc_rans_encode: bits 0-7 the element size (1, 2 or 4), bits 8-15 the filter, every higher bit 0.
 * A plain 1, 2 or 4 is therefore what it always was: no filter, a version-1 stream.  RPCC_RANS_FILTER_DELTA (format version 2,
 * magic 'R' 'B') codes the zigzagged differences of consecutive elements, each chunk on its own; a stream that does not get
 * smaller than 12 + n that way is written as the version-1 stored stream.  Any other word is refused with RPCC_RANS_E_CAPACITY.
 * The decoder takes no such word: a stream says what it is. */
#define RPCC_RANS_FILTER_NONE 0
#define RPCC_RANS_FILTER_DELTA 1
#define RPCC_RANS_WIDTH_WORD(width, filter) ((int32_t)(width) | (int32_t)(filter) << 8)
#define RPCC_RANS_WIDTH_OF(word) ((int32_t)(word) & 0xFF)
#define RPCC_RANS_FILTER_OF(word) ((int32_t)(word) >> 8 & 0xFF)

/* Per-stream results of rpcc_rans_decode (status) and rpcc_rans_encode (dst_len < 0). */
#define RPCC_RANS_OK 0
#define RPCC_RANS_E_CAPACITY (-1)   /* n (decode) or 12 + n (encode) larger than the stream's capacity; a length, width or work buffer out of range (encode) */
#define RPCC_RANS_E_HEADER (-2)     /* bad magic, mode, width, chunk_log2, filter or reserved bytes; n above RPCC_RANS_MAX_INPUT; a coded stream of no bytes */
#define RPCC_RANS_E_TRUNCATED (-3)  /* the stream ends inside the header, a table or the directory */
#define RPCC_RANS_E_TABLE (-4)      /* a table's count out of range or wrong for its plane, symbols not ascending, frequencies not summing to 4096 */
#define RPCC_RANS_E_DIRECTORY (-5)  /* the payload lengths (or a stored stream's n) do not end exactly at the end of the stream */
#define RPCC_RANS_E_STATE (-6)      /* a chunk ends with a lane's state other than 2^16 or with words left over */
#define RPCC_RANS_E_PAYLOAD (-7)    /* a chunk's payload is shorter than its states, of odd length, or runs out of words */
/* A stream's chunk-level status is the lowest of its chunks' statuses. */

int rpcc_rans_version(void);
const char *rpcc_rans_last_error(void);

/* Worst-case size of one stream: 12 + n, the stored form (0 for n < 0 or n > RPCC_RANS_MAX_INPUT). */
size_t rpcc_rans_bound(int64_t n);

/* Bytes of the work buffer rpcc_rans_encode takes for nstreams streams of total_bytes bytes together (any upper bound of the sum
 * of their lengths) at chunk_log2 (0 for an invalid argument).
 * Caller's buffers: ws needs no initialisation (it may hold anything, an earlier call's contents included), nothing outside the
 * size above is touched and its contents are undefined on return; align it to 16 bytes.  dst is written only where a stream lands:
 * dst[dst_off[s] .. + dst_len[s]) -- the rest of a slot, the gaps between slots and a refused stream's slot are left as they are.
 * dst_len and status are written for every stream. */
size_t rpcc_rans_workspace_bytes(int64_t nstreams, int64_t total_bytes, int chunk_log2);

/* Encode nstreams streams.  src_ptr (dev, uint64 [nstreams]) device addresses, src_len (dev, int64) their lengths, width (dev,
 * int32 [nstreams]; null: every stream 1) their width words -- the element size 1, 2 or 4, or RPCC_RANS_WIDTH_WORD; stream s is written at dst + dst_off[s] (dev, int64), which
 * must have room for dst_cap[s] (dev, int64) >= rpcc_rans_bound(src_len[s]) bytes.  total_bytes: what rpcc_rans_workspace_bytes was
 * given.  dst_len (dev, int64 [nstreams]): bytes written, or RPCC_RANS_E_CAPACITY when the length or width is out of range, the slot
 * too small or the lengths add up to more than total_bytes (nothing is written then).  A stream whose coded form would not be smaller
 * than 12 + n is stored. */
int rpcc_rans_encode(const uint64_t *src_ptr, const int64_t *src_len, const int32_t *width, int64_t nstreams, int64_t total_bytes,
                     int chunk_log2, uint8_t *dst, const int64_t *dst_off, const int64_t *dst_cap, int64_t *dst_len, void *ws, void *stream);

/* Decode nstreams streams (src_ptr, src_len as for encode) into dst + dst_off[s], at most dst_cap[s] bytes.  status (dev, int32
 * [nstreams]): RPCC_RANS_OK or one of RPCC_RANS_E_*; dst_len (dev, int64): n when OK, else 0.  A refused stream writes nothing: every
 * chunk is checked (decoded without stores) before the first byte of its stream is written. */
int rpcc_rans_decode(const uint64_t *src_ptr, const int64_t *src_len, int64_t nstreams, uint8_t *dst, const int64_t *dst_off,
                     const int64_t *dst_cap, int64_t *dst_len, int32_t *status, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* RPCC_RANS_H */
