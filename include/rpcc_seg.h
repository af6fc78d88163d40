/*
 * rpcc_seg.h -- C ABI of librpcc_seg.so: DBSCAN segmentation on the MI355X (gfx950), the device counterpart of the
 * reference's segment_method 'DBSCAN' (utils/segment_utils.py:149-169, Open3D cluster_dbscan).  A library of its own,
 * apart from librpcc_hip.so.
 *
 * Conventions as in rpcc_eval.h: plain pointers and sizes; every pointer marked "dev" is a device pointer; kernels are
 * enqueued on the caller's hipStream_t (passed as void*) and nothing synchronises; the library allocates nothing (work
 * buffer: rpcc_seg_workspace_bytes); 0 = OK, negative = error with the text in rpcc_seg_last_error().  Argument errors
 * return RPCC_SEG_ERR_ARG before anything touches the device.
 *
 * Per frame: a pixel is non-ground when |double(ri) - r_plane| > 0.5 in fp64, r_plane = -d / ((a*A + b*B) + c*C) (a NaN
 * residual is ground; zero-range pixels count).  Points are the fp32 products ri * tm, ranked row-major over the
 * non-ground pixels.  q is a neighbour of p when ((dx*dx) + (dy*dy)) + (dz*dz) < eps*eps in fp64, un-fused, with
 * dx = double(xp) - double(xq); the point itself counts.  Core points have >= min_points neighbours; clusters are the
 * components of core points, numbered 0, 1, ... by their lowest core rank; a non-core point takes the lowest cluster
 * number among its core neighbours, else it is noise.  DESIGN.md section 10 states the whole specification.
 */
#ifndef RPCC_SEG_H
#define RPCC_SEG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RPCC_SEG_ABI_VERSION 1
#define RPCC_SEG_ERR_ARG (-1)
#define RPCC_SEG_ERR_HIP (-2)
#define RPCC_SEG_MAX_BATCH 65535       /* frames per call: the frame index is a grid dimension */
#define RPCC_SEG_MAX_PIXELS (1 << 26)  /* H*W per frame */
#define RPCC_SEG_BRUTEFORCE 1          /* flag: every candidate is tested in fp64, no pruning, no early exit (the tests' reference) */
#define RPCC_SEG_NSTATS 2              /* int64 per frame in stats: pair tests, tiles visited (all passes) */
#define RPCC_SEG_CAPPED (-1)           /* max_label[b] when a union-find loop hit its iteration cap (never for valid input) */

int rpcc_seg_version(void);
const char *rpcc_seg_last_error(void);

/* Bytes of the work buffer rpcc_seg_dbscan takes for a batch of B frames of H x W (0 for an invalid shape). */
size_t rpcc_seg_workspace_bytes(int B, int H, int W);

/* DBSCAN segmentation of B frames.  ri (dev, f32 [B,H,W]) range images; tm (dev, f32 [H,W,3]) the transform map shared by
 * the batch; ground (dev, f64 [B,4]) plane a, b, c, d per frame; eps > 0 the radius; min_points >= 1.
 * seg (dev, int32 [B,H,W]): the reference's final labels -- ground 0, noise 2, cluster k -> k + 3, then every ri == 0
 * pixel 1.  max_label (dev, int32 [B]): the largest label of each frame, RPCC_SEG_CAPPED if the frame's union-find hit
 * its iteration cap.  stats (dev, int64 [B,2], may be NULL): pair tests and tiles visited per frame.
 * flags: RPCC_SEG_BRUTEFORCE. */
/* Caller's buffers: ws needs no initialisation -- it may hold anything, a previous call's contents under another shape included --, nothing
 * outside rpcc_seg_workspace_bytes(B, H, W) bytes of it is touched and its contents are undefined on return.  Align it to 16 bytes (the
 * point table at its start holds 16-byte elements); the tests use 256, and base + 16 once.  seg and max_label are written completely and repeat bit for bit.
 * stats are written for every frame too, but they count work, and how much a workgroup does depends on the order in which its lanes list
 * the tiles: they may differ from run to run (the labels do not). */
int rpcc_seg_dbscan(const float *ri, const float *tm, const double *ground, int B, int H, int W, double eps, int min_points,
                    int flags, int32_t *seg, int32_t *max_label, int64_t *stats, void *ws, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* RPCC_SEG_H */
