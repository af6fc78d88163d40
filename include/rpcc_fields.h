/*
 * rpcc_fields.h -- C ABI of librpcc_fields.so: the point records of .pcd / .ply files unpacked to stored rows on the MI355X (gfx950),
 * the device counterpart of the Open3D read the reference's DatasetTemplate.load_data does for these files (dataset/dataset.py:43-63)
 * and of its float32 cast.  A library of its own, apart from librpcc_hip.so.
 *
 * Conventions as in rpcc_records.h: plain pointers and sizes; every pointer marked "dev" is a device pointer; the kernel is enqueued
 * on the caller's hipStream_t (passed as void*) and nothing synchronises; the library allocates nothing and takes no work buffer;
 * 0 = OK, negative = error with the text in rpcc_fields_last_error().  Argument errors return RPCC_FIELDS_ERR_ARG before anything
 * touches the device.
 *
 * A frame is described by RPCC_FIELDS_DESC_WORDS int64 words (the layout rpcc_amd/pointfile.py makes of a file's header):
 *   [0] span_off   [1] span_bytes   the frame's body inside `bytes`, any alignment
 *   [2] n                           its points
 *   [3..6]  off[x, y, z, w]         byte of point 0's element, relative to span_off
 *   [7..10] step[x, y, z, w]        bytes from one point's element to the next
 *   [11..14] type[x, y, z, w]       RPCC_FIELDS_T_*; w (the intensity) may be NONE
 *   [15] reserved
 * Element c of point i is the size(type_c) little-endian bytes at bytes + span_off + off_c + i * step_c.  Strided records
 * (array of structures: every step is the record size) and planes (structure of arrays: step = size) are the same form.
 * The row rule -- F32 as it is, F64 and the integers through one round-to-nearest-even conversion to fp32, NONE = +0.0 -- is
 * csrc_fields/fields_rule.h; DESIGN.md section 25 states the whole specification.
 */
#ifndef RPCC_FIELDS_H
#define RPCC_FIELDS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RPCC_FIELDS_ABI_VERSION 1
#define RPCC_FIELDS_ERR_ARG (-1)
#define RPCC_FIELDS_ERR_HIP (-2)
#define RPCC_FIELDS_DESC_WORDS 16
#define RPCC_FIELDS_MAX_STEP 256             /* bytes from one element to the next, at most */
#define RPCC_FIELDS_MAX_TOTAL 2147483647     /* rows per call: what the batch calls take as `total` */
#define RPCC_FIELDS_MAX_BATCH 1048576        /* frames per call */

#define RPCC_FIELDS_T_NONE 0
#define RPCC_FIELDS_T_F32 1
#define RPCC_FIELDS_T_F64 2
#define RPCC_FIELDS_T_I8 3
#define RPCC_FIELDS_T_U8 4
#define RPCC_FIELDS_T_I16 5
#define RPCC_FIELDS_T_U16 6
#define RPCC_FIELDS_T_I32 7
#define RPCC_FIELDS_T_U32 8

#define RPCC_FIELDS_OK 0          /* status[b] */
#define RPCC_FIELDS_E_LAYOUT 1    /* the descriptor names bytes outside its span, a step below the size or above MAX_STEP, an unknown type,
                                     a missing x / y / z, or a row count other than row_offsets[b+1] - row_offsets[b] */

int rpcc_fields_version(void);
const char *rpcc_fields_last_error(void);

/* Unpacks the B frames of a chunk in one launch.
 * bytes (dev): the chunk, nbytes bytes, 16-byte aligned; the files stand in it wherever the caller put them.
 * desc (dev, i64 [B, RPCC_FIELDS_DESC_WORDS]); row_offsets (dev, i64 [B+1]): frame b's rows are rows[row_offsets[b] .. row_offsets[b+1]),
 * row_offsets[0] == 0, non-decreasing, row_offsets[B] == total.  rows (dev, f32 [total,4]): 16-byte aligned, the stored-row layout every
 * entry of librpcc_hip.so reads with point_stride_bytes = 16.  status (dev, i32 [B]).
 * 0 <= B <= RPCC_FIELDS_MAX_BATCH, 0 <= total <= RPCC_FIELDS_MAX_TOTAL, nbytes >= 0; with B == 0 nothing is launched.  rows must not
 * overlap bytes.
 * The kernel validates a frame before it reads a byte of it; a frame that fails gets status RPCC_FIELDS_E_LAYOUT and rows of +0.0, no
 * value of its descriptor is used as an address, and every other frame is unaffected.  No address outside bytes .. bytes + nbytes is
 * read.  Exactly total * 16 bytes of rows and B * 4 of status are written, whatever they held before; the result repeats bit for bit.
 * (A frame whose row_offsets pair is itself out of order or outside 0 .. total gets E_LAYOUT and none of its rows are written.) */
int rpcc_fields_unpack(const void *bytes, int64_t nbytes, const int64_t *desc, int B, const int64_t *row_offsets, int64_t total,
                       float *rows, int32_t *status, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* RPCC_FIELDS_H */
