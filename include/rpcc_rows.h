/*
 * rpcc_rows.h -- C ABI of librpcc_rows.so: a decoded batch turned into the rows of the .bin files on the MI355X (gfx950), the device
 * counterpart of the reference's save rule (dataset/dataset.py:72-107, restated in DatasetTemplate.save_point_cloud_to_file).  A library
 * of its own, apart from librpcc_hip.so; the counterpart of librpcc_records.so, which makes input rows.
 *
 * Conventions as in rpcc_records.h: plain pointers and sizes; every pointer marked "dev" is a device pointer; the kernels are enqueued
 * on the caller's hipStream_t (passed as void*) and nothing synchronises; the library allocates nothing; 0 = OK, negative = error with
 * the text in rpcc_rows_last_error().  Argument errors return RPCC_ROWS_ERR_ARG before anything touches the device.
 *
 * The rule (tests/rows_ref.py): pixel p of frame b, pc[b][p] = (x, y, z), is kept iff s = (x + y) + z, computed in
 * fp32, un-fused, in that order, is != 0 -- NaN and inf - inf are kept, (1.5, -1.5, 0) is dropped, as the reference does.  The kept
 * pixels in ascending pixel order become rows (x, y, z, w) of four float32, bits unchanged; w = intensity[b][p], or +0.0 without one.
 */
#ifndef RPCC_ROWS_H
#define RPCC_ROWS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RPCC_ROWS_ABI_VERSION 1
#define RPCC_ROWS_ERR_ARG (-1)
#define RPCC_ROWS_ERR_HIP (-2)
#define RPCC_ROWS_MAX_BATCH 65535          /* frames per call */
#define RPCC_ROWS_MAX_PIXELS (1 << 26)     /* P per frame; and B * P < 2^31 */
#define RPCC_ROWS_ROUND 4096               /* pixels one workgroup ranks per round (1024 lanes x 4 consecutive pixels) */
/* int64 words of the offsets table of a call with B frames: [0 .. B] the offsets, [B + 1] the status word (RPCC_ROWS_OK or
 * RPCC_ROWS_E_CAPACITY), [B + 2 .. 2B + 1] the frames' own row counts, which the first launch hands to the second.  One D2H copy of
 * the first B + 2 words brings offsets and status together. */
#define RPCC_ROWS_TABLE_WORDS(B) (2 * (size_t)(B) + 2)
#define RPCC_ROWS_OK 0
#define RPCC_ROWS_E_CAPACITY 1             /* the batch keeps more rows than rows_capacity: nothing of rows was written */

int rpcc_rows_version(void);
const char *rpcc_rows_last_error(void);

/* Packs B frames of P pixels.
 *   pc (dev, f32 [B,P,3]): the decoded points in raster order.  intensity (dev, f32 [B,P]) or NULL: the rows' fourth column.
 *   ri_rec (dev, f32 [B,P]) or NULL: the decoded range image, read for nonzero only.
 *   rows (dev, f32 [rows_capacity,4]): 16-byte aligned; may be NULL with rows_capacity 0.  Frame b occupies rows[offsets[b] : offsets[b+1]],
 *     the frames back to back; offsets[0] = base.  Exactly offsets[B] - base rows are written and no byte outside them; what rows held
 *     before does not matter; the result repeats bit for bit.
 *   rows_capacity: in rows, >= 0; B * P always suffices.  If base + the batch's rows exceed it, nothing of rows is written, the offsets are
 *     still the true ones and the status word is RPCC_ROWS_E_CAPACITY.
 *   offsets (dev, i64 [RPCC_ROWS_TABLE_WORDS(B)]): the table above, written completely; no other scratch is taken.
 *   nonzero (dev, i32 [B]) or NULL: the pixels of each frame with ri_rec != 0 (NaN counts); needs ri_rec.
 *   base (dev, i64 [1]) or NULL: the row the first frame starts at, read on the device when the second launch runs -- the offsets[B] of
 *     an earlier call on the same stream, so that the chunks of a batch follow one another without the host knowing their sizes.  NULL: 0.
 * 1 <= B <= RPCC_ROWS_MAX_BATCH, 1 <= P <= RPCC_ROWS_MAX_PIXELS, B * P < 2^31.  Two launches, one workgroup per frame each. */
int rpcc_rows_pack(const float *pc, const float *intensity, const float *ri_rec, int B, int P, float *rows, int64_t rows_capacity,
                   int64_t *offsets, int32_t *nonzero, const int64_t *base, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* RPCC_ROWS_H */
