/*
 * rpcc_hip.h -- C ABI of librpcc_hip.so: the MI355X (gfx950) implementation of the R-PCC per-frame
 * compression hot path.  Plain pointers and sizes only; every pointer marked "dev" is a device
 * (HBM) pointer, every kernel is enqueued on the caller's hipStream_t (passed as void*) and the call
 * returns without synchronising unless stated.  The library allocates nothing: work buffers come
 * from the caller (rpcc_workspace_bytes).  Return value: 0 = OK, negative = error
 * (rpcc_last_error() gives the text); nothing throws or exits across this boundary.
 *
 * Each entry point names the reference interface it replaces (paths relative to the reference
 * repository).  A "frame" is one LiDAR sweep; a batch holds B frames of one lidar geometry (H x W
 * range image, P = H*W pixels); M = cluster_num (cfgs/compressor.yaml:22); labels are
 * 0 = ground, 1 = empty pixel, 2..M+1 = FPS cluster k-2 (utils/segment_utils.py:168-169), K = M+2.
 */
#ifndef RPCC_HIP_H
#define RPCC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RPCC_OK 0
#define RPCC_ERR_ARG (-1)
#define RPCC_ERR_HIP (-2)
#define RPCC_MAX_CLUSTERS 254 /* labels are stored as uint8 (more clusters: the rpcc_*_wide entries below) */
#define RPCC_MAX_BATCH 65535   /* frames per call: the frame index is a grid dimension */
#define RPCC_INFO_INTS 8       /* int32 per frame in the `info` arrays below */
#define RPCC_FPS_BRUTEFORCE 1  /* flag: farthest point sampling by the one-pass-per-centre kernel (test reference) */
/* The two things of the reference's CUDA binary that its source leaves to the compiler / the reduction tree (no golden vector
 * exists for either; measured effect on the selected centres: profiles/r03_fps_mode_sensitivity.md -- none in 305 frames).
 * Default (no flag): un-fused distance, lowest index among exactly equal values.  A mode flag runs the reference's own
 * algorithm (one pass per centre), about 16x the time of the pruned kernel. */
#define RPCC_FPS_FMA1 2        /* distance of sampling_gpu.cu:64 contracted as nvcc --fmad=true may: fma(dz,dz,fma(dx,dx,dy*dy)) */
#define RPCC_FPS_FMA2 4        /* ... or fma(dz,dz,fma(dy,dy,dx*dx)) */
#define RPCC_FPS_TIE_CUDA 8    /* winner among exactly equal values = the survivor of the kernel's shared-memory tree
                                  (sampling_gpu.cu:16-21,55-69,74-134): smallest bit-reversed (k mod block), then smallest k */

/* Re-entrancy: the library keeps no per-call state of its own (a cache of kernel attributes already set, behind a
 * mutex, is all it holds); every call works on the caller's buffers and stream, so host threads may call concurrently
 * on different streams with different buffers (the reference's ThreadPoolExecutor front-end,
 * tools/compress_datalist.py:202-206).  The one developer hook that is process-wide is rpcc_debug_stamps. */

/* Caller's buffers (held by tests/test_gpu_buffers.py: exact sizes, hostile contents, guard bytes around them).
 * Work buffers -- `ws`, `scratch`, `fps_table`, sized by rpcc_workspace_bytes[_general], rpcc_wide_workspace_bytes,
 * rpcc_project_scratch_bytes, rpcc_fps_table_bytes, rpcc_plane_workspace_bytes, rpcc_codec_workspace_bytes, rpcc_decompress_workspace_bytes, rpcc_labels_workspace_bytes,
 * rpcc_project_beams_scratch_bytes, rpcc_compress_batch_beams_workspace_bytes -- need NO initialisation: they
 * may hold anything, including what an earlier call left there under other arguments (another B, P, M, point count or entry point), and a
 * buffer larger than asked for may be handed to calls of different shapes in turn.  Every entry clears or overwrites what it reads; the
 * fused batch compares its per-frame projection flags with a mark kept inside ws, and a stale word that happens to equal the mark only
 * sends that frame through the exact input-order projection (slower, same result).  Their contents are undefined on return, except where a
 * stage hands them to the next (the stages of rpcc_compress_batch_stages on one ws; fps_table from rpcc_ground_mask to rpcc_fps_range).
 * No entry reads or writes a byte outside the size it asked for.  Alignment: the base must be aligned to 16 bytes (the layouts place their
 * parts at offsets that are multiples of 4 .. 256 bytes RELATIVE to the base and read some with 16-byte loads); 256 bytes -- what
 * hipMalloc and torch give -- is what the tests use, but for one run of every kind of work buffer at base + 16.
 * Outputs are written completely by every call, whatever they held before, and identically when the call is repeated, except:
 *   q16 / q32 [b, nnz[b]:]            entries past a frame's count are left as they are (the caller need not zero them)
 *   idx_sequence [b, nseq[b]:]        likewise (rpcc_contour_encode)
 *   packed [total:]                   likewise (rpcc_pack_payload)
 *   pc_rec, pred, inliers, q16 / q32  where NULL is allowed, NULL means not written
 *   salience, key_point_map           not touched in the uniform framework (rpcc_batch_io.nonuniform == NULL); complete otherwise
 * In particular every row of model / counts (labels without pixels too), all RPCC_INFO_INTS ints of info and the pad bits of the last
 * byte of contour_bits are written. */

/* Interface version: changes whenever the layout of a struct below or the meaning of an argument changes (the structs carry no size
 * field).  A binding compares rpcc_version() with the RPCC_ABI_VERSION of the header it was built against before it calls anything else
 * (r-pcc_amd/_lib.py does).  100: round 3.  101: rpcc_batch_io.point_stride_bytes.  102: the uint16-label entries (rpcc_*_wide), rpcc_compress_batch_stages.
 * 103: the scanner-order window projection entry, the RPCC_PROJECT_* bits of rpcc_batch_io.flags, the uint16 stage entries (rpcc_assign_wide ...).
 * 104: the window projection entry and the RPCC_PROJECT_* bits removed (rpcc_batch_io.flags takes the FPS bits only).
 * 105: rpcc_decompress_batch, rpcc_decompress_batch_wide, rpcc_decompress_workspace_bytes and the RPCC_STREAM_* status codes.
 * (rpcc_compress_batch_labels, rpcc_labels_workspace_bytes, rpcc_labels_io and the RPCC_LABELS_* codes were added under 105: they leave every
 * struct and argument that existed as it was, and a binding that needs them finds a library without them when it resolves its symbols.) */
#define RPCC_ABI_VERSION 105
int rpcc_version(void);
const char *rpcc_last_error(void);

/* Lidar geometry: the scalars PCTransformer.__init__ derives from a lidar YAML
 * (dataset/transformer.py:26-37); the three angles are the python doubles narrowed to C float
 * exactly as pybind11 does at cpp_modules.cpp:427-428. */
typedef struct rpcc_geom {
    int32_t H, W;
    float horizontal_fov, vertical_max, vertical_min; /* radians */
} rpcc_geom;

/* ---- a2: spherical projection ------------------------------------------------------------- *
 * replaces dataset_utils_cpp.point_cloud_to_range_image_even (cpp_modules.cpp:427-467), batched.
 *   xyz      dev f32 [total,3]   points of all frames back to back (AoS, as np.fromfile gives)
 *   offsets  dev i64 [B+1]       frame b owns points offsets[b]..offsets[b+1]
 *   total    host                offsets[B]
 *   ri       dev f32 [B,P]  out  min positive depth per pixel, 0 where empty
 *   scratch  dev, scratch_bytes  work buffer (contents undefined on return).  With
 *            rpcc_project_scratch_bytes(total,B,P) bytes the LDS-band path runs (about 40 bytes of address
 *            space per point for images of up to four 32768-pixel bands -- the records are binned by
 *            chunk of 2048 points and band in fixed shares, 6 bytes per point are touched); with at least
 *            B*(P+8)*4 bytes, or an image of more than eight bands, the device-atomic path runs (same result).
 * Exact reference semantics incl. a depth-0 point resetting its pixel in input order.  Points
 * whose depth is not finite are skipped (reference: undefined behaviour).
 * The pixel of a point is first computed by a screened fast path and recomputed with the exact
 * operation sequence whenever it is not provably the same (DESIGN.md "Projection").
 * rpcc_project_fastpath_check (test hook): counts dev u64[5] = {points the fast path is certain
 * about, of those the ones whose pixel differs from the exact sequence (must be 0), points sent
 * to the exact sequence, largest |fast - exact| of the pre-rounding column and row coordinate in
 * units of 1e-9 over the points of ordinary magnitude}. */
size_t rpcc_project_scratch_bytes(int64_t total, int B, int P);
int rpcc_project_fastpath_check(const float *xyz, int64_t total, rpcc_geom g, uint64_t *counts, void *stream);
int rpcc_project(const float *xyz, const int64_t *offsets, int64_t total, int B, rpcc_geom g, float *ri,
                 void *scratch, size_t scratch_bytes, void *stream);
/* The same on the points AS STORED: the reference reads a sweep as np.fromfile(path, float32).reshape(-1, 4) -- rows
 * (x, y, z, intensity) -- and slices [:, :3] on the host (dataset/dataset.py:48-50,62).  With point_stride_bytes = 16 the
 * rows go to the device as they are (file -> pinned buffer -> DMA, no host pass over the points) and the kernel reads one
 * 16-byte row per point (points 16-byte aligned); 12 (or 0) = packed xyz = rpcc_project.  offsets / total count POINTS. */
int rpcc_project_strided(const float *points, int point_stride_bytes, const int64_t *offsets, int64_t total, int B,
                         rpcc_geom g, float *ri, void *scratch, size_t scratch_bytes, void *stream);

/* ---- a2 through a per-beam elevation table ---------------------------------------------------- *
 * replaces the channel_distribute_csv branch of PCTransformer.point_cloud_to_range_image (dataset/transformer.py:13-22,68-91),
 * batched: the lidars whose beams are not evenly spaced in elevation.  Row h of the image is entry h of the table (radians, f64;
 * any order, equal entries allowed).  Per point, in input order (the specification is stated once, in tests/beam_table_ref.py):
 *   depth = sqrtf(x*x + y*y + z*z); a point whose depth is not finite is skipped
 *   az = atan2f(y, x), + (float)(2 pi) in fp32 when negative;  col = rintf(az / horizontal_fov * W) (half to even) mod W
 *   el = atan2f(z, sqrtf(x*x + y*y));  row = the FIRST minimum over h of |table[h] - (double)el| in fp64
 *   ri[row, col] = depth: the LAST point in input order wins its pixel (a depth-0 point that comes last leaves 0); empty pixels are 0
 * (added under interface version 105, as rpcc_compress_batch_labels was: no existing struct or argument changes)
 *
 * The index: built on the host (pure C: no device call, no allocation) into `out`, rpcc_beam_index_bytes(H) bytes, 8-byte aligned;
 * the caller uploads it once per lidar and passes the device copy (8-byte aligned) as beams_dev.  It holds the table in row order,
 * the table sorted, the fp32 midpoints of neighbouring sorted entries and the sorted-position -> row map (equal entries: the lowest
 * row); layout in csrc/beam_index.h.  1 <= H <= 128 and every entry finite, or RPCC_ERR_ARG (rpcc_beam_index_bytes: 0).  An index
 * must be used with the H it was built for.
 *   geom     H, W and horizontal_fov (> 0) are used; vertical_max / vertical_min are ignored
 *   points   packed xyz (point_stride_bytes 0 or 12) or the stored 16-byte rows, as for rpcc_project_strided; total < 2^31
 *   scratch  dev, rpcc_project_beams_scratch_bytes(total, B, P) bytes (4 per pixel + 4 per point); needs no initialisation
 * The pixel of a point comes from a screened fast path (the elevation located among the fp32 midpoints) and is recomputed by the
 * exact sequence above whenever it is not provably the same.
 * rpcc_project_beams_check (test hook; packed xyz): counts dev u64[3] = {points the fast path is certain about, of those the ones
 * the exact sequence skips or puts into another pixel (must be 0), points sent to the exact sequence}. */
#ifndef RPCC_BEAM_MAX_H
#define RPCC_BEAM_MAX_H 128 /* rows of a per-beam elevation table */
#endif
size_t rpcc_beam_index_bytes(int H);
int rpcc_beam_index_build(const double *angles, int H, void *out);
size_t rpcc_project_beams_scratch_bytes(int64_t total, int B, int P);
int rpcc_project_beams(const float *points, int point_stride_bytes, const int64_t *offsets, int64_t total, int B, rpcc_geom g,
                       const void *beams_dev, float *ri, void *scratch, size_t scratch_bytes, void *stream);
int rpcc_project_beams_check(const float *xyz, int64_t total, rpcc_geom g, const void *beams_dev, uint64_t *counts, void *stream);

/* ---- intensity: the fourth column of the stored rows, one byte per non-empty pixel ------------- *
 * The reference drops the column (dataset/dataset.py:62); these entries carry it beside the geometry.  The specification is stated
 * once, in tests/intensity_ref.py (added under interface version 105: new exports only, no existing struct or argument changes):
 *   owner     per frame, rows i = 0 .. N-1 in input order: d_i = sqrtf(x*x + y*y + z*z) un-fused, rows of non-finite d_i skipped, pix_i the
 *             pixel of rpcc_project.  The reference's loop `if (ri[pix] == 0 || d < ri[pix]) ri[pix] = d` gains `own[pix] = i`; a pixel is
 *             non-empty iff its final ri != 0 and its owner is the final own.  In closed form: z = the last i with pix_i == pix and
 *             d_i == 0 (or -1); the owner is the smallest i > z with pix_i == pix and the bits of d_i equal to the bits of ri[pix].
 *   quantise  r = rintf(w * scale) (one fp32 multiply, half to even); q = 0 unless r >= 0 (NaN, negatives), 255 if r > 255, else (uint8)r
 *   dequant   w' = (float)q / scale, one correctly rounded fp32 division (scale 100 returns a KITTI sweep's k / 100 bit for bit)
 *   payload   8 + n bytes: "RPI1", scale as little-endian f32, then q of the non-empty pixels in ascending pixel index; n = pixels with
 *             ri != 0 = pixels whose label is not 1, which is what the decoder has
 * rpcc_intensity_encode: rows dev f32 [total,4] (16-byte aligned), offsets dev i64 [B+1], ri dev f32 [B,P] the image rpcc_project made of
 * these rows; scale finite and > 0.  Out: payload dev u8 rows of payload_stride >= 8 + P bytes (frame b: 8 + n_b bytes are written, the rest
 * is left as it is), nbytes dev i32 [B] = 8 + n_b, image dev u8 [B,P] or NULL (q per pixel, 0 where empty), owner_intensity dev f32 [B,P] or NULL (the owner's fourth float as stored, 0
 * where empty: what --eval compares the decoded values with), orphans dev i32 [B] = non-empty
 * pixels no row owns (0 whenever ri is the image of these rows; such a pixel is coded as 0).  scratch: rpcc_intensity_scratch_bytes(B, P)
 * bytes (8 per pixel + flags; needs no initialisation).  One device atomic per candidate owner; minima only, so the result does not depend
 * on scheduling.
 * rpcc_intensity_decode: payload rows / nbytes as above, labels dev [B,P] of label_bytes 1 (uint8) or 2 (uint16).  Out: intensity dev f32
 * [B,P], 0 where the label is 1; status dev i32 [B] = RPCC_STREAM_OK, or RPCC_STREAM_E_INTENSITY when nbytes[b] is outside 8 .. the row,
 * the magic is missing, the scale is not finite and > 0, or nbytes[b] - 8 is not the number of labels != 1: that frame's row is zeros and
 * its payload is never used as an index.
 * Both queue on `stream` and do not synchronise; argument errors (NULL, unaligned rows, total outside 0 .. 2^31 - 1, B outside
 * 1 .. RPCC_MAX_BATCH, a geometry the projection refuses, a bad scale, a small scratch or row stride, another label_bytes) return
 * RPCC_ERR_ARG before the device is touched. */
size_t rpcc_intensity_scratch_bytes(int B, int P);
int rpcc_intensity_encode(const float *rows, const int64_t *offsets, int64_t total, int B, rpcc_geom g, const float *ri, float scale,
                          uint8_t *payload, int64_t payload_stride, int32_t *nbytes, uint8_t *image, float *owner_intensity, int32_t *orphans,
                          void *scratch, size_t scratch_bytes, void *stream);
int rpcc_intensity_decode(const uint8_t *payload, int64_t payload_stride, const int32_t *nbytes, const void *labels, int label_bytes, int B,
                          int P, float *intensity, int32_t *status, void *stream);

/* ---- subpixel: where inside its cell a pixel's owner lies, 1 .. 4 bits per axis ---------------- *
 * A decoded point lies on the centre ray of its pixel; these entries carry the offset the projection rounds away.  The specification is
 * stated once, in tests/subpixel_ref.py (new exports under interface version 105; no existing struct or argument changes):
 *   owner     the intensity channel's: the row whose depth the projection keeps (above)
 *   offsets   the owner's x, y, z through the projection's fp32 sequence: off_az = colf - roundf(colf), taken before the column wraps (a
 *             point that rounds to column W has column 0 and a negative offset); off_el = rowf - (float)row, taken after the row is
 *             clamped to 0 .. H-1 (so it may lie outside +-0.5)
 *   code      L = 1 << bits; t = (off + 0.5f) * (float)L (one fp32 add, one fp32 multiply); c = min(max((int)floorf(t), 0), L - 1);
 *             it stands for the offset (c + 0.5) / L - 0.5 cells
 *   payload   8 + 2n bytes: "RPS1", bits, three zero bytes, the az codes of the non-empty pixels in ascending pixel index, then their el
 *             codes; one byte per code; n = pixels with ri != 0 = pixels whose label is not 1
 * rpcc_subpixel_encode: rows / offsets / ri as rpcc_intensity_encode takes them; bits 1 .. 4.  Out: payload dev u8 rows of payload_stride
 * >= 8 + 2P bytes (frame b: 8 + 2 n_b bytes are written, the rest is left as it is), nbytes dev i32 [B] = 8 + 2 n_b, codes dev u8 [B,P,2]
 * (2-byte aligned) or NULL: (az, el) per pixel, 0 where empty; orphans dev i32 [B] = non-empty pixels no row owns (coded as 0, 0).
 * scratch: rpcc_subpixel_scratch_bytes(B, P) bytes, no initialisation needed.
 * rpcc_subpixel_decode: labels dev [B,P] of label_bytes 1 or 2, ri_rec dev f32 [B,P] the reconstructed ranges, tables dev f64
 * [2H + 2W + 256]: cos / sin of the rows' altitudes (ca [H], sa [H]) and of the columns' azimuths (cz [W], sz [W]) as the transform map is
 * built from them, then for bits = 1 .. 4 and code c = 0 .. 15 at ((bits - 1) * 16 + c) * 4: cos, sin of the elevation step
 * ((c + 0.5) / L - 0.5) * vfov / (H-1) and cos, sin of the azimuth step ((c + 0.5) / L - 0.5) * hfov / W.  Out: points dev f32 [B,P,3]:
 *   cosalt = ca*cde - sa*sde; sinalt = sa*cde + ca*sde; cosaz = cz*cda - sz*sda; sinaz = sz*cda + cz*sda          (fp64, un-fused)
 *   x = (float)((double)r * (cosalt * cosaz)); y = (float)((double)r * (cosalt * sinaz)); z = (float)((double)r * sinalt)
 * and +0.0 where the label is 1; status dev i32 [B] = RPCC_STREAM_OK, or RPCC_STREAM_E_SUBPIXEL (the frame's points are zeros, no code is
 * used as an index) when nbytes[b] is outside 8 .. the row, the magic is missing, bits is outside 1 .. 4, a reserved byte is not 0,
 * nbytes[b] != 8 + 2 (labels != 1), or any code is >= L.
 * Argument errors return RPCC_ERR_ARG before the device is touched, as for the intensity entries; besides, H * W must stay below
 * 2^30 - 4, so that 8 + 2 H W, the longest payload, fits the int32 of nbytes (rpcc_subpixel_scratch_bytes returns 0 above it). */
#define RPCC_STREAM_E_SUBPIXEL 11 /* rpcc_subpixel_decode */
size_t rpcc_subpixel_scratch_bytes(int B, int P);
int rpcc_subpixel_encode(const float *rows, const int64_t *offsets, int64_t total, int B, rpcc_geom g, const float *ri, int bits,
                         uint8_t *payload, int64_t payload_stride, int32_t *nbytes, uint8_t *codes, int32_t *orphans, void *scratch,
                         size_t scratch_bytes, void *stream);
int rpcc_subpixel_decode(const uint8_t *payload, int64_t payload_stride, const int32_t *nbytes, const void *labels, int label_bytes,
                         const float *ri_rec, const double *tables, int H, int W, int B, float *points, int32_t *status, void *stream);

/* ---- hidden_points: the points that share a pixel with its owner ---------------------------------- *
 * The range image keeps one point per pixel; these entries carry the others.  The specification is stated once, in tests/hidden_ref.py
 * (new exports under interface version 105; no existing struct or argument changes):
 *   skipped   a row whose depth from the projection's sequence is NaN, infinite or 0, as rpcc_project skips it
 *   owner     the intensity channel's (above); every other row whose pixel is non-empty is a hidden point of that pixel -- a row of equal
 *             depth bits that comes later, a row in front of a later depth-0 row of its pixel (it may be nearer than the owner)
 *   range     k = rintf(d / step), one IEEE fp32 division, half to even; a point with !(k <= 65535) is not carried; the decoded range is
 *             (float)k * step, one fp32 multiply: |r - d| <= step * (0.5 + k * 2^-23)
 *   lateral   bits 0 .. 4; for bits > 0 the subpixel codes of the point's own off_az / off_el against its pixel, else 0
 *   order     key = k << 8 | az << 4 | el; by pixel in raster order, then by key; at most the 255 smallest keys of a pixel are carried
 *   uncarried hidden points in an empty pixel (ri == 0), with k past 65535 or past the 255 of their pixel: counted per frame, never an error
 *   payload   "RPH1", bits, three zero bytes, step as little-endian f32, m as little-endian u32, one count byte per non-empty pixel in
 *             raster order [n], the k values as little-endian u16 [m], and for bits > 0 the az codes [m] and the el codes [m]:
 *             16 + n + 2m bytes, or 16 + n + 4m
 * rpcc_hidden_encode: rows / offsets / ri as rpcc_intensity_encode takes them; step finite and > 0; bits 0 .. 4.  Out: payload dev u8 rows
 * of payload_stride >= 16 + P bytes -- 16 + P + 4 N holds every frame of at most N rows; a frame whose payload is longer than the row
 * gets nbytes -1 and only its header and count plane are written --, nbytes dev i32 [B], orphans dev i32 [B] as for the subpixel entry,
 * uncarried dev i32 [B].  scratch: rpcc_hidden_scratch_bytes(B, P, total) bytes, no initialisation needed.  Atomics count and hand out
 * slots only; the bytes do not depend on scheduling.
 * rpcc_hidden_decode: labels dev [B,P] of label_bytes 1 or 2, tm dev f32 [P,3] the transform map (bits 0: r * tm, the multiply of
 * rpcc_backproject), tables as rpcc_subpixel_decode takes them or NULL (bits > 0: the pixel's ray turned by the two offsets through the
 * same fp64 expressions).  Out: points dev f32 [B, capacity, 3], frame b's m_b points in payload order, the rest left as it is; count dev
 * i32 [B] = m_b; status dev i32 [B] = RPCC_STREAM_OK, or RPCC_STREAM_E_HIDDEN (count 0, no point written, no byte used as an index) unless
 * 16 <= nbytes[b] <= payload_stride, the magic matches, bits <= 4 and the reserved bytes are 0, step is finite and > 0, the labels other
 * than 1 number n, nbytes[b] is the length above, the counts sum to m, m <= capacity, every az / el code is below 2^bits, and tables is
 * not NULL when bits > 0.
 * Argument errors return RPCC_ERR_ARG before the device is touched, as for the subpixel entries; besides, 16 + P + 4 total must stay
 * below 2^31 (rpcc_hidden_scratch_bytes returns 0 above it). */
#define RPCC_STREAM_E_HIDDEN 12 /* rpcc_hidden_decode */
size_t rpcc_hidden_scratch_bytes(int B, int P, int64_t total);
int rpcc_hidden_encode(const float *rows, const int64_t *offsets, int64_t total, int B, rpcc_geom g, const float *ri, float step, int bits,
                       uint8_t *payload, int64_t payload_stride, int32_t *nbytes, int32_t *orphans, int32_t *uncarried, void *scratch,
                       size_t scratch_bytes, void *stream);
int rpcc_hidden_decode(const uint8_t *payload, int64_t payload_stride, const int32_t *nbytes, const void *labels, int label_bytes,
                       const float *tm, const double *tables, int H, int W, int B, float *points, int64_t capacity, int32_t *count,
                       int32_t *status, void *stream);

/* ---- a4: ground plane ----------------------------------------------------------------------- *
 * replaces the ground branch of PointCloudSegment.segment: candidate selection + RANSAC
 * (utils/segment_utils.py:74-82,101-108).  The reference uses Open3D segment_plane on an unseeded
 * np.random.choice subsample (third-party, random); this is the build's deterministic seeded
 * definition (DESIGN.md "RANSAC"): z < -1.5 candidates, systematic subsample to 5000, all pixels if
 * fewer than 800, 100 hypotheses of 10 points, 0.1 m inlier distance, refit on the inliers.
 *   frame_ids dev i64 [B] or NULL a stable identity per frame (its datalist index): frame b draws with
 *                                seed + (uint32)frame_ids[b] (NULL: seed + b), so a file's plane -- and its
 *                                bitstream -- does not depend on the batch it travels in
 *   ground   dev f64 [B,4] out   plane a,b,c,d (unit normal) per frame
 *   inliers  dev i32 [B]   out   inlier count of the winning hypothesis (may be NULL)            */
int rpcc_ground_ransac(const float *ri, const float *tm, int B, int P, uint32_t seed, const int64_t *frame_ids,
                       double *ground, int32_t *inliers, void *stream);

/* ---- a3+a5: back-projection + vertical ground residual + FPS state init -------------------- *
 * replaces PCTransformer.range_image_to_point_cloud (dataset/transformer.py:94-101) and
 * PointCloudSegment.calc_plane_residual_vertical cpu branch + mask (utils/segment_utils.py:44-47,
 * 119-120).  Candidates (depth_dif > threshold) get temp = 1e10 (ops/fps/fps_utils.py:26), all other
 * pixels temp = -1 (never selectable).
 *   ri       dev f32 [B,P]
 *   tm       dev f32 [P,3]       transform_map (dataset/transformer.py:41-54)
 *   ground   dev f64 [B,4]       plane a,b,c,d per frame
 *   temp     dev f32 [B,P]  out
 *   info     dev i32 [B,8]  out  {n_left, first candidate pixel (P if none), nnz, fps_table valid,
 *                                 first EMPTY pixel that is a candidate (P if none), 3 spare}       */
int rpcc_ground_mask(const float *ri, const float *tm, const double *ground, double threshold, int B, int H, int W,
                     float *temp, int32_t *info, void *fps_table, void *stream);
/* fps_table (optional, rpcc_fps_table_bytes(B,H,W) bytes, or NULL): when given, the kernel also runs the
 * first pass of the farthest point sampling (distance of every candidate to the first centre, per-tile
 * bounding boxes and maxima) and temp holds min(1e10, that distance) for frames with info[b][3] == 1;
 * pass the same table to rpcc_fps_range.  Results are identical with and without it. */
size_t rpcc_fps_table_bytes(int B, int H, int W);

/* ---- a6: farthest point sampling ----------------------------------------------------------- *
 * rpcc_fps_xyz replaces furthest_point_sampling_wrapper(b,n,m,points,temp,idx)
 * (ops/fps/src/sampling.cpp:24-37, kernel ops/fps/src/sampling_gpu.cu:24-140): same arguments, same
 * caller-initialised temp (1e10), idx[b][0] = 0, strict '>' arg-max, ties -> lowest index.
 *   points dev f32 [B,N,3], temp dev f32 [B,N] in/out, idx dev i32 [B,M] out                      */
int rpcc_fps_xyz(int B, int N, int M, const float *points, float *temp, int32_t *idx, void *stream);

/* rpcc_fps_range is the same sampling run directly on the range image (xyz = ri * tm recomputed in
 * registers; pixels with temp < 0 are not candidates).  It selects the pixels the reference selects
 * on the compacted candidate list (utils/segment_utils.py:120-124).
 *   temp     dev f32 [B,P] in/out from rpcc_ground_mask (candidates share one initial value, others < 0); on return
 *                                the running minimum distance of every candidate, as the reference kernel leaves it
 *   info     dev i32 [B,8]       from rpcc_ground_mask (first candidate = start point; first empty candidate)
 *   cen_pix  dev i32 [B,M]  out  pixel index of each centre
 *   centers  dev f32 [B,M,3] out cluster_centers
 *   flags    0, or RPCC_FPS_BRUTEFORCE for the one-pass-per-centre kernel (identical results), or the CUDA-binary modes
 *            RPCC_FPS_FMA1 / RPCC_FPS_FMA2 / RPCC_FPS_TIE_CUDA (fps_table must be NULL then; k of the tie rule = rank of
 *            the pixel among the candidates, block = opt_n_threads(n_left))                              */
int rpcc_fps_range(const float *ri, const float *tm, float *temp, const int32_t *info, int B, int H, int W, int M,
                   int32_t *cen_pix, float *centers, int flags,
                   const void *fps_table /* from rpcc_ground_mask, or NULL */, void *stream);

/* The brute-force form of rpcc_fps_xyz (one full pass per centre): the test reference of the tile-pruned kernels. */
int rpcc_fps_xyz_bruteforce(int B, int N, int M, const float *points, float *temp, int32_t *idx, void *stream);
/* rpcc_fps_xyz with flags: RPCC_FPS_BRUTEFORCE, RPCC_FPS_FMA1 / RPCC_FPS_FMA2, RPCC_FPS_TIE_CUDA (k = the point's index,
 * block = opt_n_threads(N) as sampling_gpu.cu:9-13 computes it). */
int rpcc_fps_xyz_mode(int B, int N, int M, const float *points, float *temp, int32_t *idx, int flags, void *stream);
/* rpcc_fps_xyz sends every list to the kernel its point order suits: tiles of 256 consecutive points that are compact in space (the reference's
 * row-major candidate list, a sweep in its stored order) -> the tile-pruned kernel; no locality (a shuffled cloud) -> one pass per centre.  Same
 * indices either way.  Test hook: the decision alone.   marks dev i32 [B] out: -1 = one pass per centre, 0 = tile-pruned */
int rpcc_fps_xyz_probe(int B, int N, const float *points, int32_t *marks, void *stream);

/* ---- a7: ground / cluster assignment + relabel ---------------------------------------------- *
 * replaces calc_plane_residual_depth, calc_cluster_residual_radius, concatenate + argmax and the
 * relabel (utils/segment_utils.py:21-23,64-67,127-131,168-169).
 *   seg      dev u8 [B,P] out labels                                                              */
int rpcc_assign(const float *ri, const float *tm, const double *ground, const float *centers, int B, int H, int W,
                int M, uint8_t *seg, void *stream);

/* ---- a8: point model ------------------------------------------------------------------------- *
 * replaces segment_utils_cpp.point_modeling (cpp_modules.cpp:471-518) + the model_param assembly
 * (utils/segment_utils.py:183-185, tools/compress.py:102), then the pybind11 fp64->fp32 cast.
 *   model    dev f32 [B,K,4] out row 0 = (float)ground, row 1 = 0, row k = [0,0,0,mean_k]
 *                                (NaN 0xFFC00000 for a label without pixels)
 *   counts   dev i32 [B,K]   out pixels per label
 *   ws       dev, rpcc_workspace_bytes                                                            */
int rpcc_point_model(const float *ri, const uint8_t *seg, const double *ground, int B, int P, int M, float *model,
                     int32_t *counts, void *ws, void *stream);

/* ---- a9: plane model --------------------------------------------------------------------------- *
 * replaces cluster_modeling('plane') (utils/segment_utils.py:188-216) incl. plane_angle_validation
 * (:84-93) and the fp32 numpy-mean fallbacks.  RANSAC (ransac_n = 4, 10 iterations, 0.1 m) is the
 * build's seeded specification (Open3D in the reference); label k of frame b uses hash(seed, id_b, k) with
 * id_b = frame_ids[b] (dev i64 [B]) or b when frame_ids is NULL.
 *   inject_planes dev f64 [B,K,4] or NULL: test hook -- row (b,k) replaces the RANSAC result of label k (what the
 *            fixtures of tests/golden/pins_*.npz do to the reference through ransac_plane_segmentation), so that the
 *            angle validation and the mean fallbacks can be compared with the genuine cluster_modeling('plane')
 *   ground   dev f64 [B,4] or NULL   copied (as fp32) into row 0
 *   cos_cut  HOST double: a plane is rejected when some pixel has |n.t|/|n|*|t| <= cos_cut, i.e.
 *            arccos(.) > angle threshold; the caller derives it from its own arccos (ops.plane_model)
 *   model    dev f32 [B,K,4] out;  counts dev i32 [B,K] out;  ws rpcc_plane_workspace_bytes(B,P,M)   */
size_t rpcc_plane_workspace_bytes(int B, int P, int M);
int rpcc_plane_model(const float *ri, const float *tm, const uint8_t *seg, const double *ground, int B, int P, int M,
                     double cos_cut, uint32_t seed, const int64_t *frame_ids, const double *inject_planes, float *model,
                     int32_t *counts, void *ws, void *stream);

/* ---- a10+a11(+a13): intra-prediction + residual + quantisation + ordered scatter ------------- *
 * replaces segment_utils_cpp.intra_predict (cpp_modules.cpp:248-285), residual = ri - pred
 * (tools/compress.py:106), quantization_utils_cpp.uniform_quantize (cpp_modules.cpp:288-334) and the
 * quantising half of nonuniform_quantize (cpp_modules.cpp:404-422).
 *   acc         quantisation step (= 2*accuracy, tools/compress.py:46) as C float (uniform)
 *   label_acc   dev f32 [B,K] per-label step from rpcc_salience (non-uniform), or NULL
 *   residual_in dev f32 [B,P] residual supplied by the caller (QuantizationModule.quantize_residual's
 *               own argument, utils/compress_utils.py:57), or NULL to compute ri - pred here.  With
 *               residual_in given and pred == NULL nothing is predicted: ri, tm and model may be NULL
 *               (exactly uniform_quantize(seg_idx, residual, acc), cpp_modules.cpp:288)
 *   q16         dev i16 [B,P] out   per frame: nnz values grouped by label ascending, row-major inside
 *                                   a label, already cast to int16 (utils/compress_utils.py:142)
 *   q32         dev i32 [B,P] out   same as int32 (what the quantisers return); either may be NULL
 *   nnz         dev i32 [B]   out
 *   pred        dev f32 [B,P] out   optional (NULL to skip)                                          */
int rpcc_predict_quantize(const float *ri, const float *tm, const uint8_t *seg, const float *model,
                          const float *label_acc, const float *residual_in, float acc, int B, int P, int M,
                          int16_t *q16, int32_t *q32, int32_t *nnz, float *pred, void *ws, void *stream);

/* a10 alone: segment_utils_cpp.intra_predict (cpp_modules.cpp:248-285) -> pred dev f32 [B,P]. */
int rpcc_intra_predict(const uint8_t *seg, const float *model, const float *tm, int B, int P, int M, float *pred,
                       void *stream);

/* ---- a12: key points ---------------------------------------------------------------------------- *
 * replaces feature_extractor_cpp.extract_features_with_segment (cpp_modules.cpp:28-121, mark_as_picked
 * :10-25) with zero-initialised outputs (the reference leaves unwritten cells uninitialised).
 *   feat          dev f32 [B,H,W] out   curvature feature
 *   key_point_map dev u8  [B,H,W] out   0 none, 1 flat, 2 less sharp, 3 sharp
 * Limits: W <= 4096 (a row lives in one workgroup's registers / LDS), 1 <= feature_region <= 16, segments >= 1;
 * any chunk length (W / segments) and any sharp / less_sharp / flat counts.                            */
int rpcc_extract_features(const float *ri, const uint8_t *seg, int B, int H, int W, int feature_region, int segments,
                          int sharp_num, int less_sharp_num, int flat_num, float *feat, uint8_t *key_point_map,
                          void *stream);

/* ---- a13: salience levels ------------------------------------------------------------------------ *
 * replaces the per-label level selection of nonuniform_quantize (cpp_modules.cpp:355-405).
 *   level_kp_num HOST i32 [levels], level_acc HOST f32 [levels]  (base step + delta, compress_utils.py:48)
 *   salience   dev u8  [B,K] out   level per label;  label_acc dev f32 [B,K] out  its step            */
int rpcc_salience(const uint8_t *seg, const uint8_t *key_point_map, const int32_t *level_kp_num, const float *level_acc,
                  int levels, int ground_level, int B, int P, int M, uint8_t *salience, float *label_acc, void *stream);

/* ---- a3: back-projection as its own entry --------------------------------------------------- *
 * replaces PCTransformer.range_image_to_point_cloud (dataset/transformer.py:94-101).
 *   pc       dev f32 [B,P,3] out  ri[...,None] * transform_map                                     */
int rpcc_backproject(const float *ri, const float *tm, int B, int P, float *pc, void *stream);

/* ---- f1: contour map + index sequence --------------------------------------------------------- *
 * replaces contour_utils_cpp.extract_contour (cpp_modules.cpp:521-558) and the casts/packing of
 * compress_point_cloud (utils/compress_utils.py:156-160).
 *   contour_bits dev u8  [B, ceil(P/8)] out  np.packbits(contour_map) (first pixel = MSB)
 *   idx_sequence dev u16 [B,P]          out  labels at the contour positions, row-major; nseq[b] entries
 *   ws           dev, rpcc_codec_workspace_bytes(B,P,M)                                            */
size_t rpcc_codec_workspace_bytes(int B, int P, int M);
int rpcc_contour_encode(const uint8_t *seg, int B, int H, int W, uint8_t *contour_bits, uint16_t *idx_sequence,
                        int32_t *nseq, void *ws, void *stream);

/* ---- f3: decoder ------------------------------------------------------------------------------- *
 * rpcc_contour_decode replaces np.unpackbits + contour_utils_cpp.recover_map (cpp_modules.cpp:561-593,
 * utils/compress_utils.py:202-206).
 * rpcc_decode replaces QuantizationModule.dequantize_residual (utils/compress_utils.py:114-132),
 * intra_predict, range_image_rec = pred + residual and range_image_to_point_cloud
 * (tools/decompress.py:88-112).
 *   q16        dev i16 [B,P]   label-ordered quantised residuals (as stored in the bitstream)
 *   model      dev f32 [B,K,4] plane_param from the bitstream
 *   level_acc  HOST f64 [max(levels,1)]  quantisation step(s): uniform -> levels = 0 and level_acc[0]
 *   salience   dev u8 [B,K]    per-label level (non-uniform only)
 *   ri_rec     dev f32 [B,P] out ;  pc_rec dev f32 [B,P,3] out (may be NULL)                        */
int rpcc_contour_decode(const uint8_t *contour_bits, const uint16_t *idx_sequence, int B, int H, int W, uint8_t *seg,
                        void *ws, void *stream);
int rpcc_decode(const uint8_t *seg, const int16_t *q16, const float *model, const float *tm, const double *level_acc,
                int levels, const uint8_t *salience, int B, int P, int M, float *ri_rec, float *pc_rec, void *ws,
                void *stream);

/* ---- f2: the batch's residual stream, frames back to back ------------------------------------ *
 * replaces the per-frame `residual_quantized` arrays of compress_point_cloud (utils/compress_utils.py:142,160)
 * for a batch: packed = concat_b q16[b][:nnz[b]] (prefix sums taken on the device; no host round trip).
 *   q16      dev i16 [B,P]   label-ordered residuals (rpcc_predict_quantize / rpcc_compress_batch)
 *   nnz      dev i32 [B]     entries per frame
 *   packed   dev i16 [capacity] out   entries past `capacity` are dropped (capacity >= sum of the frames' input
 *                                     points is always enough: a pixel holds at least one point)
 *   total    dev i64 [1] out (may be NULL)  sum of nnz = entries written
 * What a rank hands to the D2H copy or to the RCCL gather of payloads instead of the padded array. */
int rpcc_pack_payload(const int16_t *q16, const int32_t *nnz, int B, int P, int16_t *packed, int64_t capacity,
                      int64_t *total, void *stream);

/* ---- fused batch entry: a2..a13 for B frames (FPS segmentation; uniform / non-uniform framework; point / plane model) *
 * The batched counterpart of the body of tools/compress.py:93-125 /
 * tools/compress_datalist.py:91-125 with the ground model supplied by the caller or fitted inside. */
/* QuantizationModule's non-uniform settings (utils/compress_utils.py:36-54, cfgs/compressor.yaml:26-36) */
typedef struct rpcc_nonuniform_cfg {
    int32_t levels;              /* 1..8 */
    int32_t level_kp_num[8];     /* level_key_point_num */
    float level_acc[8];          /* base step + level_delta_acc, as C float (utils/compress_utils.py:48) */
    int32_t ground_level;        /* ground_salience_level */
    int32_t feature_region, segments, sharp_num, less_sharp_num, flat_num;
} rpcc_nonuniform_cfg;

typedef struct rpcc_batch_io {
    const float *xyz;        /* dev f32 [total,3] (or [total,4] rows with point_stride_bytes = 16) */
    const int64_t *offsets;  /* dev i64 [B+1] */
    int64_t total;
    const float *tm;         /* dev f32 [P,3] */
    double *ground;          /* dev f64 [B,4]  in (ground_seed < 0: injected models) / out (fitted here) */
    int64_t ground_seed;     /* >= 0: fit the ground plane with rpcc_ground_ransac(seed = ground_seed, frame_ids) */
    const int64_t *frame_ids;/* dev i64 [B] or NULL: stable identity of every frame (seeds; see rpcc_ground_ransac) */
    float *ri;               /* dev f32 [B,P] out */
    uint8_t *seg;            /* dev u8  [B,P] out */
    int32_t *cen_pix;        /* dev i32 [B,M] out */
    float *centers;          /* dev f32 [B,M,3] out */
    float *model;            /* dev f32 [B,K,4] out */
    int32_t *counts;         /* dev i32 [B,K] out */
    int16_t *q16;            /* dev i16 [B,P] out */
    int32_t *nnz;            /* dev i32 [B] out */
    int32_t *info;           /* dev i32 [B,8] out */
    int32_t flags;           /* 0, RPCC_FPS_BRUTEFORCE, or the CUDA-binary FPS modes RPCC_FPS_FMA1 / _FMA2 / _TIE_CUDA; any other bit is
                                refused (RPCC_ERR_ARG) */
    void *timer;             /* rpcc_timer_create() handle or NULL: times this call's FPS launch (bench.py) */
    /* framework / model selection (tools/compress.py:109-124, cfgs/compressor.yaml: compress_framework, modeling_method) */
    int32_t model_method;    /* 0: point model (a8);  1: plane model (a9: rpcc_plane_model with plane_cos_cut, plane_seed,
                                frame_ids); ws must then hold rpcc_workspace_bytes_general() bytes */
    double plane_cos_cut;    /* see rpcc_plane_model */
    int64_t plane_seed;
    const rpcc_nonuniform_cfg *nonuniform; /* HOST, NULL: uniform framework (step = acc); else key points + salience
                                levels + per-label steps (a12, a13), ws of rpcc_workspace_bytes_general() bytes */
    uint8_t *salience;       /* dev u8 [B,K] out (non-uniform) */
    uint8_t *key_point_map;  /* dev u8 [B,P] out (non-uniform) */
    int32_t point_stride_bytes; /* bytes per point of `xyz`: 0 or 12 = packed xyz; 16 = (x, y, z, intensity) rows as stored in a
                                KITTI .bin (see rpcc_project_strided) */
} rpcc_batch_io;

size_t rpcc_workspace_bytes(int B, int P, int M, int64_t total_points);
size_t rpcc_workspace_bytes_general(int B, int P, int M, int64_t total_points); /* plane model and / or non-uniform framework */
int rpcc_compress_batch(const rpcc_batch_io *io, int B, rpcc_geom g, int M, double ground_threshold, float acc,
                        void *ws, void *stream);

/* rpcc_compress_batch with the projection stage replaced by rpcc_project_beams (beams_dev: the device copy of the index built for g.H);
 * everything behind the projection reads io->ri and io->tm -- the ray table built from the same elevation table -- and is unchanged:
 * all four framework / model combinations, byte labels up to RPCC_MAX_CLUSTERS clusters and uint16 labels (io->seg) up to
 * RPCC_MAX_CLUSTERS_MID.  ws: rpcc_compress_batch_beams_workspace_bytes(B, P, M, total_points, general) bytes (general != 0: plane
 * model and / or non-uniform framework; 0 for a batch this entry does not take).  The mixed-geometry call and cluster counts above
 * RPCC_MAX_CLUSTERS_MID have no table form. */
size_t rpcc_compress_batch_beams_workspace_bytes(int B, int P, int M, int64_t total_points, int general);
int rpcc_compress_batch_beams(const rpcc_batch_io *io, int B, rpcc_geom g, const void *beams_dev, int M, double ground_threshold,
                              float acc, void *ws, void *stream);

/* A subset of rpcc_compress_batch's stages, in order: bit 0 projection, 1 ground fit, 2 mask (+ first FPS pass), 3 FPS, 4 assignment + label histograms +
 * scan (+ the plane model's label order), 5 plane fits, 6 key points + salience + quantiser.  For callers that interleave the stages of several batches on
 * several streams themselves; every stage needs the stages before it to have run on the same io / ws.  All bits (127) = rpcc_compress_batch. */
#define RPCC_STAGE_ALL 127
int rpcc_compress_batch_stages(const rpcc_batch_io *io, int B, rpcc_geom g, int M, double ground_threshold, float acc, void *ws,
                               int stage_mask, void *stream);

/* The same for a batch that holds sweeps of several lidar geometries (variable H x W inside one call: BASELINE configs[4]; the
 * reference compresses such a list frame by frame with one dataset / transformer per lidar, tools/compress_datalist.py:160-206,
 * the YAML files of dataset/lidar_cfg).  The frames are grouped by geometry: group i = ios[i] (its own buffers, laid out for Bs[i] frames of
 * geoms[i], exactly as for rpcc_compress_batch), workspace wss[i] of rpcc_workspace_bytes[_general](Bs[i], P_i, M, total_i) bytes.
 * Everything is queued on `stream`; the kernels with one workgroup per frame or per label (ground RANSAC, FPS, plane fits) run
 * as ONE launch over the frames of all groups, the pixel-parallel kernels group after group.  Results per group are what
 * rpcc_compress_batch returns for that group alone.  G <= RPCC_MAX_GROUPS; ground_seed / model_method / nonuniform may differ
 * between the groups. */
#define RPCC_MAX_GROUPS 4
int rpcc_compress_batch_mixed(const rpcc_batch_io *ios, const int *Bs, const rpcc_geom *geoms, int G, int M,
                              double ground_threshold, float acc, void *const *wss, void *stream);

/* cluster_num above RPCC_MAX_CLUSTERS (the reference takes any value, cfgs/compressor.yaml:22; its labels travel as uint16,
 * utils/compress_utils.py:160): the same batch with `io->seg` pointing to uint16 [B,P] labels, 255 <= M <= RPCC_MAX_CLUSTERS_WIDE (smaller M work too).
 * Same stages, same arithmetic, same results as rpcc_compress_batch -- one thread per pixel or label, per-label totals by global atomics, the ordered
 * scatter through one stable radix sort of (frame, label) keys: written for correctness, not for speed (csrc/wide_kernels.h).  All four framework / model
 * combinations; the CUDA-binary FPS modes are not available here.  ws: rpcc_wide_workspace_bytes(B, P, M, total_points) bytes.
 * The container's side of it: the contour codec and the decoder body on uint16 label maps (rpcc_decode_wide: ws of rpcc_wide_workspace_bytes(B, P, M, 0)).
 * rpcc_decode_wide takes label maps of foreign streams: a label above M + 1 (no row of `model`) is read as M + 1 -- memory-safe, the pixel's value is then
 * meaningless as the stream's was; callers that must reject such a stream check the label range first (compress_utils.decode_frame does). */
#define RPCC_MAX_CLUSTERS_WIDE 65533
/* Up to RPCC_MAX_CLUSTERS_MID clusters the per-label tables of the tuned kernels still fit LDS: rpcc_compress_batch_wide then runs the assignment, the
 * label histogram, the plane model's label order and the quantiser of rpcc_compress_batch on uint16 labels (250 k frames/s at 300 clusters against
 * 89 k through the radix sort), and the reference's STAGE seams exist for such counts too -- the uint16 forms of rpcc_assign, rpcc_point_model, rpcc_intra_predict
 * and rpcc_predict_quantize (same arguments, `seg` as uint16; ws of rpcc_workspace_bytes(B, P, M, 0) bytes):
 * PointCloudSegment.segment / cluster_modeling('point') / intra_predict and the uniform quantize_residual stage by stage at cluster_num 255 .. 1022. */
#define RPCC_MAX_CLUSTERS_MID 1022
int rpcc_assign_wide(const float *ri, const float *tm, const double *ground, const float *centers, int B, int H, int W, int M, uint16_t *seg, void *stream);
int rpcc_point_model_wide(const float *ri, const uint16_t *seg, const double *ground, int B, int P, int M, float *model, int32_t *counts, void *ws, void *stream);
int rpcc_plane_model_wide(const float *ri, const float *tm, const uint16_t *seg, const double *ground, int B, int P, int M, double cos_cut, uint32_t seed,
                          const int64_t *frame_ids, const double *inject_planes, float *model, int32_t *counts, void *ws, void *stream);
int rpcc_intra_predict_wide(const uint16_t *seg, const float *model, const float *tm, int B, int P, int M, float *pred, void *stream);
int rpcc_extract_features_wide(const float *ri, const uint16_t *seg, int B, int H, int W, int feature_region, int segments, int sharp_num,
                               int less_sharp_num, int flat_num, float *feat, uint8_t *key_point_map, void *stream);
int rpcc_salience_wide(const uint16_t *seg, const uint8_t *key_point_map, const int32_t *level_kp_num, const float *level_acc, int levels,
                       int ground_level, int B, int P, int M, uint8_t *salience, float *label_acc, void *stream);
int rpcc_predict_quantize_wide(const float *ri, const float *tm, const uint16_t *seg, const float *model, const float *label_acc, const float *residual_in,
                               float acc, int B, int P, int M, int16_t *q16, int32_t *q32, int32_t *nnz, float *pred, void *ws, void *stream);
size_t rpcc_wide_workspace_bytes(int B, int P, int M, int64_t total_points);
int rpcc_compress_batch_wide(const rpcc_batch_io *io, int B, rpcc_geom g, int M, double ground_threshold, float acc, void *ws, void *stream);
int rpcc_contour_encode_wide(const uint16_t *seg, int B, int H, int W, uint8_t *contour_bits, uint16_t *idx_sequence, int32_t *nseq, void *ws, void *stream);
int rpcc_contour_decode_wide(const uint8_t *contour_bits, const uint16_t *idx_sequence, int B, int H, int W, uint16_t *seg, void *ws, void *stream);
int rpcc_decode_wide(const uint16_t *seg, const int16_t *q16, const float *model, const float *tm, const double *level_acc, int levels,
                     const uint8_t *salience, int B, int P, int M, float *ri_rec, float *pc_rec, void *ws, void *stream);

/* ---- the batch from a caller's label map: a8..a13 for B frames whose segmentation exists already ------------------------------------ *
 * The stages of rpcc_compress_batch behind its assignment, entered with int32 labels in rpcc_seg_dbscan's convention (include/rpcc_seg.h;
 * the reference's segment_method 'DBSCAN', utils/segment_utils.py:149-169): ground 0, ri == 0 pixels 1, noise 2, clusters from 3.  M is a label
 * CAP, not a cluster count: frame b uses the labels 0 .. max_label[b], and these must be <= M + 1; K = M + 2 rows per frame as everywhere.
 * M <= RPCC_MAX_CLUSTERS: byte labels, the kernels of rpcc_compress_batch; up to RPCC_MAX_CLUSTERS_MID: uint16 labels, the same kernels as
 * rpcc_compress_batch_wide runs for such counts; above: RPCC_ERR_ARG.  One pass over the int32 labels (the label intake) writes the narrow map
 * `seg`, checks every label against min(max_label[b], M + 1) and leaves the per-tile label counts -- for the point model the per-label range
 * sums too -- that the label histogram would otherwise read `seg` again for; point or plane model, key points and salience levels, prediction
 * and quantiser follow as in rpcc_compress_batch.  Everything is queued on `stream`; nothing synchronises.
 *   ws       dev, rpcc_labels_workspace_bytes(B, P, M, general) bytes (general != 0: plane model and / or non-uniform framework); needs no
 *            initialisation, like every work buffer (see "Caller's buffers")
 * A frame is REFUSED when max_label[b] is RPCC_LABELS_CAPPED (what rpcc_seg_dbscan writes as RPCC_SEG_CAPPED), negative or above M + 1, or when
 * one of its labels lies outside 0 .. max_label[b]: its status is RPCC_LABELS_E_CAPPED / RPCC_LABELS_E_RANGE, every output row of it (seg,
 * model, counts, all P entries of q16, salience, key_point_map) is zero bytes and nnz[b] = 0; none of its labels is used as an index.  The
 * other frames of the batch are what they are without it. */
#define RPCC_LABELS_CAPPED (-1)
#define RPCC_LABELS_OK 0
#define RPCC_LABELS_E_RANGE 1
#define RPCC_LABELS_E_CAPPED 2
typedef struct rpcc_labels_io {
    const float *ri;          /* dev f32 [B,P] */
    const float *tm;          /* dev f32 [P,3] */
    const double *ground;     /* dev f64 [B,4] */
    const int32_t *labels;    /* dev i32 [B,P] */
    const int32_t *max_label; /* dev i32 [B] */
    const int64_t *frame_ids; /* dev i64 [B] or NULL (the plane model's seeds; see rpcc_plane_model) */
    void *seg;                /* dev u8 [B,P] (M <= RPCC_MAX_CLUSTERS) or u16 [B,P] out */
    float *model;             /* dev f32 [B,K,4] out */
    int32_t *counts;          /* dev i32 [B,K] out */
    int16_t *q16;             /* dev i16 [B,P] out */
    int32_t *nnz;             /* dev i32 [B] out */
    int32_t *status;          /* dev i32 [B] out: RPCC_LABELS_OK or RPCC_LABELS_E_* */
    int32_t model_method;     /* as in rpcc_batch_io, with plane_cos_cut / plane_seed */
    double plane_cos_cut;
    int64_t plane_seed;
    const rpcc_nonuniform_cfg *nonuniform; /* HOST, or NULL: uniform framework */
    uint8_t *salience;        /* dev u8 [B,K] out (non-uniform) */
    uint8_t *key_point_map;   /* dev u8 [B,P] out (non-uniform) */
} rpcc_labels_io;
size_t rpcc_labels_workspace_bytes(int B, int P, int M, int general);
int rpcc_compress_batch_labels(const rpcc_labels_io *io, int B, rpcc_geom g, int M, float acc, void *ws, void *stream);

/* ---- f3 for a batch of streams: the decoding counterpart of rpcc_compress_batch ------------------------------------------------ *
 * Takes the decoded payloads of B frames where the entropy decoders left them -- every row padded to the geometry's maximum -- and gives label maps,
 * range images and points: the host checks of tools/decompress.py:decode_frame as one status per frame, then rpcc_contour_decode and rpcc_decode
 * for the frames that pass.  Everything is queued on `stream`; nothing synchronises.
 *   contour_bits   dev u8  [B, ceil(P/8)]
 *   idx_sequence   dev u16 [B,P]
 *   model          dev f32 [B,K,4]
 *   q16            dev i16 [B,P]
 *   salience       dev u8  [B,K]          (NULL in the uniform framework: levels == 0)
 *   payload_len    dev i64 [B,5]          decoded byte counts in container order: salience_level, contour_map, idx_sequence, plane_param,
 *                                         residual_quantized (the salience column is ignored in the uniform framework)
 *   entropy_status dev i32 [B,5]          the entropy decoders' statuses in the same order, 0 = sound (salience column: likewise ignored)
 *   tm, level_acc (HOST f64), levels, M   as in rpcc_decode;  H, W as in rpcc_contour_decode
 *   status         dev i32 [B]     out    RPCC_STREAM_OK or RPCC_STREAM_E_*
 *   seg            dev u8  [B,P]   out    (rpcc_decompress_batch_wide: u16 [B,P], 255 <= M <= RPCC_MAX_CLUSTERS_WIDE)
 *   ri_rec         dev f32 [B,P]   out ;  pc_rec dev f32 [B,P,3] out (may be NULL)
 *   ws             dev, rpcc_decompress_workspace_bytes(B, P, M) bytes (M above RPCC_MAX_CLUSTERS: the uint16 entry's layout)
 * Whatever lies past a payload's stated length, in any input row, is not read as data: it may hold anything.  No byte outside a row is read.
 * A model row or salience entry the stream does not hold counts as zero, as decode_frame pads them.
 * The status of a frame is the first of these that applies, in decode_frame's order; rows = payload_len[plane_param] / 16:
 *   E_ENTROPY   one of the frame's entropy statuses is not 0
 *   E_PLANE     the plane payload is not a multiple of 16 bytes, or rows > K
 *   E_CONTOUR   the contour payload is not ceil(P/8) bytes
 *   E_WIDTH     the idx or the residual payload has an odd byte count
 *   E_NSEQ      the number of idx entries is not the popcount of the first P contour bits (the pad bits of the last byte do not count)
 *   E_LABEL     an idx entry is >= rows
 *   E_SALIENCE  (non-uniform) the payload is longer than K, shorter than rows, or holds a level >= levels
 *   E_RESIDUAL  the number of residual values is not the number of pixels whose recovered label is not 1
 * (a negative length fails the check of its payload).  Outputs are written completely for every frame: a refused frame's seg, ri_rec and pc_rec
 * rows are all zero bytes, and none of its payloads is used as an index.  RPCC_STREAM_E_CONTAINER is not produced here: callers that parse
 * the containers (pipeline.BatchDecompressor) give it to a frame whose length prefixes do not fit its bytes. */
#define RPCC_STREAM_OK 0
#define RPCC_STREAM_E_ENTROPY 1
#define RPCC_STREAM_E_PLANE 2
#define RPCC_STREAM_E_CONTOUR 3
#define RPCC_STREAM_E_WIDTH 4
#define RPCC_STREAM_E_NSEQ 5
#define RPCC_STREAM_E_LABEL 6
#define RPCC_STREAM_E_SALIENCE 7
#define RPCC_STREAM_E_RESIDUAL 8
#define RPCC_STREAM_E_CONTAINER 9
#define RPCC_STREAM_E_INTENSITY 10 /* rpcc_intensity_decode; callers that asked for intensity and found no (valid) trailer */
size_t rpcc_decompress_workspace_bytes(int B, int P, int M);
int rpcc_decompress_batch(const uint8_t *contour_bits, const uint16_t *idx_sequence, const float *model, const int16_t *q16, const uint8_t *salience,
                          const int64_t *payload_len, const int32_t *entropy_status, const float *tm, const double *level_acc, int levels, int B,
                          int H, int W, int M, int32_t *status, uint8_t *seg, float *ri_rec, float *pc_rec, void *ws, void *stream);
int rpcc_decompress_batch_wide(const uint8_t *contour_bits, const uint16_t *idx_sequence, const float *model, const int16_t *q16, const uint8_t *salience,
                               const int64_t *payload_len, const int32_t *entropy_status, const float *tm, const double *level_acc, int levels, int B,
                               int H, int W, int M, int32_t *status, uint16_t *seg, float *ri_rec, float *pc_rec, void *ws, void *stream);

/* Developer hook (libraries built with -DRPCC_DEVTRACE only; the shipped one returns RPCC_ERR_ARG for a non-NULL buffer):
 * register a device int64 buffer of at least RPCC_DEBUG_STAMPS_WORDS words; instrumented kernels store the shader clock at
 * phase boundaries, the FPS kernel its per-phase cycle sums and per-iteration tile counts.  NULL disables it (default). */
#define RPCC_DEBUG_STAMPS_WORDS (4096 + 16 * 128 * 8)
int rpcc_debug_stamps(void *dev_i64_buffer);

/* Timer objects for bench.py: a handle given in rpcc_batch_io.timer makes the call record hipEvents around its FPS
 * launch on the call's stream; rpcc_timer_read returns the accumulated milliseconds and the launch count since the
 * last read (synchronises the events).  One handle per measuring thread; the library keeps no global timing state.
 * rpcc_timer_reserve creates the events of the next `launches` timed launches ahead of time (event creation is not
 * cheap and would otherwise fall into the caller's timed region). */
void *rpcc_timer_create(void);
void rpcc_timer_destroy(void *timer);
int rpcc_timer_reserve(void *timer, int launches);
int rpcc_timer_read(void *timer, double *ms, int *launches);

#ifdef __cplusplus
}
#endif
#endif
