/*
 * rpcc_eval.h -- C ABI of librpcc_eval.so: reconstruction-quality metrics on the MI355X (gfx950), the
 * device counterpart of the reference's utils/evaluate_metrics.py (Chamfer distance, F-score, point-to-point
 * and point-to-plane PSNR).  A library of its own, apart from librpcc_hip.so: nothing here runs in the
 * compression step.
 *
 * Conventions as in rpcc_hip.h: plain pointers and sizes; every pointer marked "dev" is a device pointer;
 * kernels are enqueued on the caller's hipStream_t (passed as void*) and nothing synchronises; the library
 * allocates nothing (work buffer: rpcc_eval_workspace_bytes); 0 = OK, negative = error with the text in
 * rpcc_eval_last_error().  Argument errors return RPCC_EVAL_ERR_ARG before anything touches the device.
 *
 * Clouds.  A batch holds B frames; each frame is two clouds of one shape, points f32 [B,H,W,3] (a range image
 * times the transform map, ops.backproject; a point list zero-padded into rows).  A pixel holds a point when
 * ((x + y) + z) != 0 in fp32 (the reference's np.sum(p, -1) != 0).  Points are ranked by row-major pixel
 * order; every per-point array below is [B,P] (P = H*W) indexed by that rank, and only its first n entries
 * of a frame are written.  Distances are ((dx*dx) + (dy*dy)) + (dz*dz) in fp32, un-fused; among equal
 * distances the lowest rank wins.  DESIGN.md "Reconstruction metrics" states the whole specification.
 */
#ifndef RPCC_EVAL_H
#define RPCC_EVAL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RPCC_EVAL_ABI_VERSION 1
#define RPCC_EVAL_ERR_ARG (-1)
#define RPCC_EVAL_ERR_HIP (-2)
#define RPCC_EVAL_MAX_BATCH 65535       /* frames per call: the frame index is a grid dimension */
#define RPCC_EVAL_MAX_PIXELS (1 << 26)  /* H*W per frame */
#define RPCC_EVAL_BRUTEFORCE 1          /* flag: every target point is scanned, no tile pruning (the tests' reference) */
#define RPCC_EVAL_KNN 12                /* neighbours of the normal estimate (max_nn of evaluate_metrics.py:137) */
#define RPCC_EVAL_NSUMS 10              /* doubles per frame written by rpcc_eval_metrics */

int rpcc_eval_version(void);
const char *rpcc_eval_last_error(void);

/* Bytes of the work buffer every entry below takes for a batch of B frames of H x W (0 for an invalid shape). */
size_t rpcc_eval_workspace_bytes(int B, int H, int W);
/* Caller's buffers: ws needs no initialisation -- it may hold anything, e.g. what another entry of this header or a call of another shape
 * left there (one ws serves rpcc_eval_nn, rpcc_eval_normals and rpcc_eval_metrics in turn) --, nothing outside the size above is touched
 * and its contents are undefined on return.  Align it to 16 bytes (its point tables hold 16-byte elements); the tests use 256, and base + 16 once.
 * dist1 / idx1 / dist2 / idx2 and normals are indexed by rank: they are written for the n valid points of their cloud and left as they are
 * behind them; n and sums are written completely.  Everything written repeats bit for bit. */

/* Exact nearest neighbours in both directions -- the chamfer_3DDist call of calc_chamfer_distance
 * (utils/evaluate_metrics.py:9-19).  dev outputs, [B,P] by rank: dist1[i] = squared distance from cloud-1 point i
 * to its nearest cloud-2 point, idx1[i] = that point's rank; dist2 / idx2 the other way.  n (dev, int32 [B,2]):
 * points of cloud 1 and cloud 2.  A frame whose other cloud is empty gets NaN / -1.  visits (dev, int32 [B,2,P],
 * may be NULL): 8x32-pixel target tiles scanned per query, direction 1->2 then 2->1.  flags: RPCC_EVAL_BRUTEFORCE. */
int rpcc_eval_nn(const float *pts1, const float *pts2, int B, int H, int W, int flags, float *dist1, int32_t *idx1,
                 float *dist2, int32_t *idx2, int32_t *n, int32_t *visits, void *ws, void *stream);

/* Normals of one cloud -- compute_point_cloud_normal (utils/evaluate_metrics.py:133-139, Open3D
 * KDTreeSearchParamHybrid(radius=r, max_nn=12)): the eigenvector of the smallest eigenvalue of the fp64 covariance of
 * the <= 12 nearest points with d2 <= (float)(r*r), the point itself included; (0,0,1) with fewer than 3; oriented so
 * that n . p <= 0 (towards the sensor).  normals (dev, f64 [B,P,3]); nbr (dev, int32 [B,P,12], may be NULL): the
 * neighbour ranks, nearest first, -1 where there are fewer.  flags: RPCC_EVAL_BRUTEFORCE. */
int rpcc_eval_normals(const float *pts, int B, int H, int W, double r, int flags, double *normals, int32_t *nbr, void *ws,
                      void *stream);

/* Per-frame sums of calc_chamfer_distance / fscore and calc_point_to_point_plane_psnr (utils/evaluate_metrics.py:9-98,
 * assign_attr :101-117).  nn12 (dev, int32 [B,P]): rank in cloud 2 of each cloud-1 point's neighbour (Chamfer idx1, the
 * PSNR function's idx2); nn21 the other way.  normals1 (dev, f64 [B,P,3]) of cloud 1, or NULL (no point-to-plane sums).
 * sums (dev, f64 [B,10]): n1, n2, sum sqrt(d) 1->2, 2->1, sum d 1->2, 2->1, count d < threshold_sq 1->2, 2->1,
 * sum of squared point-to-plane errors 1->2, 2->1; d is recomputed from the points with the distance above, sqrt is
 * the correctly rounded fp32 sqrt, all sums are fp64.  Cloud 2's normals are the plain average of the normals of the
 * cloud-1 points whose nn12 names it (fixed-point sums: the same bits on every run), else normals1[nn21[j]].  An empty
 * cloud or an index out of range makes the frame's sums NaN. */
int rpcc_eval_metrics(const float *pts1, const float *pts2, int B, int H, int W, const int32_t *nn12, const int32_t *nn21,
                      const double *normals1, float threshold_sq, double *sums, void *ws, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* RPCC_EVAL_H */
