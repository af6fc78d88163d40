/*
 * rpcc_filter.h -- C ABI of librpcc_filter.so: radius outlier removal on the MI355X (gfx950), the device counterpart of the
 * reference's use_radius_outlier_removal (dataset/dataset.py:29-35, Open3D remove_radius_outlier(nb_points=3, radius=1)).
 * A library of its own, apart from librpcc_hip.so.
 *
 * Conventions as in rpcc_seg.h: plain pointers and sizes; every pointer marked "dev" is a device pointer; kernels are
 * enqueued on the caller's hipStream_t (passed as void*) and nothing synchronises; the library allocates nothing (work
 * buffer: rpcc_filter_workspace_bytes); 0 = OK, negative = error with the text in rpcc_filter_last_error().  Argument errors
 * return RPCC_FILTER_ERR_ARG before anything touches the device.
 *
 * Per frame: the points of the list as float32, in list order.  q is a neighbour of p when
 * ((dx*dx) + (dy*dy)) + (dz*dz) < radius*radius in fp64, un-fused, with dx = double(xp) - double(xq); the comparison is strict,
 * the point itself counts and exact duplicates are ordinary points.  A point is kept when its neighbour count is > nb_points.  A
 * point with a non-finite coordinate is removed and is nobody's neighbour.  Frames never see each other's points.  DESIGN.md
 * section 17 states the whole specification.
 */
#ifndef RPCC_FILTER_H
#define RPCC_FILTER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RPCC_FILTER_ABI_VERSION 1
#define RPCC_FILTER_ERR_ARG (-1)
#define RPCC_FILTER_ERR_HIP (-2)
#define RPCC_FILTER_MAX_BATCH 65535        /* frames per call */
#define RPCC_FILTER_MAX_POINTS (1 << 30)   /* points per call (total) */
#define RPCC_FILTER_TILE 256               /* consecutive points of one frame's list per tile, one per lane */
#define RPCC_FILTER_TILE_LIST 256          /* candidate tiles kept per round of the search's tile list (one per lane; the rounds cover any frame) */
#define RPCC_FILTER_BRUTEFORCE 1           /* flag: every point of the frame is tested in fp64, no pruning, no early exit (the tests' reference) */
#define RPCC_FILTER_NSTATS 2               /* int64 per frame in stats: pair tests, tiles visited */

int rpcc_filter_version(void);
const char *rpcc_filter_last_error(void);

/* Bytes of the work buffer rpcc_filter_radius takes for B frames of `total` points together (0 for B <= 0, B > RPCC_FILTER_MAX_BATCH,
 * total < 0 or total > RPCC_FILTER_MAX_POINTS). */
size_t rpcc_filter_workspace_bytes(int64_t total, int B);

/* Radius outlier removal of B frames.  points (dev, f32): `total` points, point_stride_bytes apart: 0 or 12 = packed x, y, z; 16 = the
 * stored rows x, y, z, intensity, whose fourth float is never interpreted.  offsets (dev, i64 [B+1]): frame b holds the points
 * offsets[b] .. offsets[b+1] - 1; offsets[0] = 0, offsets[B] = total, non-decreasing (values outside 0 .. total are clamped, so nothing outside
 * the buffers is touched whatever offsets holds; the outputs are then complete only for the points some frame covers).  total, B: host
 * values -- nothing is read back, every grid is sized from them.  radius > 0 with 1e-30 <= radius^2 <= 1e30; nb_points >= 0.
 * keep (dev, u8 [total]): 1 for a kept point, else 0.  count (dev, i32 [total], may be NULL): the neighbour count clipped at nb_points + 1
 * (0 for a non-finite point); identical with and without RPCC_FILTER_BRUTEFORCE.  kept (dev, i64 [B], may be NULL): kept points per frame.
 * masked (dev, f32, same stride and size as points, may be NULL, must not be points): a copy of the input in which x, y, z of every
 * removed point are quiet NaN (0x7fc00000); with stride 16 the fourth float is copied bit for bit.  stats (dev, i64 [B,2], may be NULL):
 * pair tests and tiles visited per frame.  flags: RPCC_FILTER_BRUTEFORCE.
 * Caller's buffers: ws needs no initialisation -- it may hold anything --, nothing outside rpcc_filter_workspace_bytes(total, B) bytes of it is
 * touched and its contents are undefined on return.  Align it to 16 bytes (the tile boxes at its start are 16-byte elements).  keep, count,
 * kept and masked are written completely and repeat bit for bit; stats count work and may differ from run to run.  With total == 0 points,
 * keep, count and masked may be NULL. */
int rpcc_filter_radius(const float *points, int point_stride_bytes, const int64_t *offsets, int64_t total, int B, double radius,
                       int nb_points, int flags, uint8_t *keep, int32_t *count, int64_t *kept, float *masked, int64_t *stats, void *ws,
                       void *stream);

#ifdef __cplusplus
}
#endif

#endif /* RPCC_FILTER_H */
