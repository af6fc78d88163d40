/*
 * rpcc_cloud.h -- C ABI of librpcc_cloud.so: a decoded batch whose frames hold image points and, behind them, a variable number of extra
 * points (the hidden_points trailer) turned into the rows of the .bin files on the MI355X (gfx950).  A library of its own beside
 * librpcc_rows.so, whose one entry it extends by the extra segment; librpcc_rows.so itself is unchanged.
 *
 * Conventions as in rpcc_rows.h: plain pointers and sizes; every pointer marked "dev" is a device pointer; the kernels are enqueued on the
 * caller's hipStream_t (passed as void*) and nothing synchronises; the library allocates nothing; 0 = OK, negative = error with the text in
 * rpcc_cloud_last_error().  Argument errors return RPCC_CLOUD_ERR_ARG before anything touches the device.
 *
 * The rule (tests/cloud_ref.py): frame b's rows are its kept pixels in raster order, then its kept extra points
 * extra[b][0 .. n_b), n_b = min(max(extra_count[b], 0), extra_capacity), in their order.  "Kept" is the rule of rpcc_rows.h for both
 * segments: s = (x + y) + z in fp32, un-fused, in that order, is != 0 -- NaN is kept, (1.5, -1.5, 0) is dropped.  A row is (x, y, z, w) of
 * four float32, the bits of x, y, z unchanged; w = intensity[b][p] for a pixel row (+0.0 without intensity) and +0.0 for an extra row: the
 * trailer carries no intensity (tools.decompress.point_intensity).
 */
#ifndef RPCC_CLOUD_H
#define RPCC_CLOUD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RPCC_CLOUD_ABI_VERSION 1
#define RPCC_CLOUD_ERR_ARG (-1)
#define RPCC_CLOUD_ERR_HIP (-2)
#define RPCC_CLOUD_MAX_BATCH 65535          /* frames per call */
#define RPCC_CLOUD_MAX_PIXELS (1 << 26)     /* P per frame, and extra_capacity per frame; and B * (P + extra_capacity) < 2^31 */
#define RPCC_CLOUD_ROUND 4096               /* points one workgroup ranks per round (1024 lanes x 4 consecutive points), in either segment */
/* int64 words of the offsets table of a call with B frames, laid out as RPCC_ROWS_TABLE_WORDS: [0 .. B] the offsets, [B + 1] the status
 * word, [B + 2 .. 2B + 1] the frames' own row counts (both segments), which the first launch hands to the second. */
#define RPCC_CLOUD_TABLE_WORDS(B) (2 * (size_t)(B) + 2)
#define RPCC_CLOUD_OK 0
#define RPCC_CLOUD_E_CAPACITY 1             /* the batch keeps more rows than rows_capacity: nothing of rows was written */

int rpcc_cloud_version(void);
const char *rpcc_cloud_last_error(void);

/* Packs B frames of P pixels and up to extra_capacity extra points each.
 *   pc, intensity, ri_rec, rows, rows_capacity, offsets, nonzero, base, stream: as rpcc_rows_pack takes them (rpcc_rows.h), with the same
 *     offsets table, status word, base chaining and E_CAPACITY behaviour -- nothing of rows is written and the offsets are still the true
 *     ones --; B * (P + extra_capacity) rows always suffice.  Exactly offsets[B] - base rows are written and no byte outside them; the
 *     result repeats bit for bit (ranks come from scans, not from atomics).  nonzero counts pixels only.
 *   extra (dev, f32 [B, extra_capacity, 3]) or NULL: the extra points; only the first n_b of frame b are read.
 *   extra_capacity: >= 0; not looked at beyond the argument checks when extra is NULL.
 *   extra_count (dev, i32 [B]): read on the device; needed whenever extra is given.
 * With extra == NULL or extra_capacity == 0 the output equals rpcc_rows_pack's, bit for bit.
 * 1 <= B <= RPCC_CLOUD_MAX_BATCH, 1 <= P <= RPCC_CLOUD_MAX_PIXELS, extra_capacity <= RPCC_CLOUD_MAX_PIXELS,
 * B * (P + extra_capacity) < 2^31.  Two launches, one workgroup per frame each. */
int rpcc_cloud_pack(const float *pc, const float *intensity, const float *ri_rec, int B, int P, float *rows, int64_t rows_capacity,
                    int64_t *offsets, int32_t *nonzero, const int64_t *base, const float *extra, int extra_capacity,
                    const int32_t *extra_count, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* RPCC_CLOUD_H */
