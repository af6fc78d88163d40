"""Reconstruction-quality metrics on the GPU -- the surface of the reference's utils/evaluate_metrics.py
(calc_chamfer_distance, calc_point_to_point_plane_psnr, psnr) on librpcc_eval.so, plus quality_batch, the same
numbers for a batch of range images in one pass with no host synchronisation.

Points are float32 (the reference's inputs are float32 point clouds); a point is valid when ((x + y) + z) != 0 in fp32
and valid points are ranked in row-major order, as the reference's np.sum(p, -1) != 0 filter ranks them.  [H,W,3]
inputs are searched as images (8x32-pixel tiles prune well on range images); [N,3] lists are zero-padded into rows of
LIST_WIDTH points, which is exact but prunes only as well as the list's order allows.  DESIGN.md "Reconstruction
metrics" has the numerical specification; nothing falls back to the CPU."""
import time

import numpy as np
import torch

from . import _eval_lib as E
from . import ops
from ._lib import RpccError, ptr, stream

LIST_WIDTH = 2048


def _points(a):
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a))
    if t.dim() not in (2, 3) or t.shape[-1] != 3:
        raise ValueError("points must be [N,3] or [H,W,3], got %s" % (tuple(t.shape),))
    return t.to(torch.float32)


def _prepare(points1, points2):
    """Both clouds as f32 [1,H,W,3] device tensors of one shape; raises ValueError naming an empty side."""
    if not torch.cuda.is_available():
        raise RpccError("the metrics run on the GPU (librpcc_eval.so); no GPU is visible")
    dev = torch.device("cuda", torch.cuda.current_device())
    a, b = _points(points1).to(dev), _points(points2).to(dev)
    if a.dim() != 3 or a.shape != b.shape:
        a, b = a.reshape(-1, 3), b.reshape(-1, 3)
        n = max(a.shape[0], b.shape[0], 1)
        w = min(LIST_WIDTH, n)
        h = -(-n // w)
        pa = torch.zeros((h * w, 3), dtype=torch.float32, device=dev)
        pb = torch.zeros((h * w, 3), dtype=torch.float32, device=dev)
        pa[: a.shape[0]] = a
        pb[: b.shape[0]] = b
        a, b = pa.view(h, w, 3), pb.view(h, w, 3)
    a, b = a.contiguous()[None], b.contiguous()[None]
    if a.shape[1] * a.shape[2] > E.MAX_PIXELS:
        raise ValueError("at most %d points (or pixels) per cloud" % E.MAX_PIXELS)
    for name, t in (("points1", a), ("points2", b)):
        if not bool(((t[..., 0] + t[..., 1]) + t[..., 2] != 0).any()):
            raise ValueError("%s holds no valid point (every point has x + y + z == 0)" % name)
    return a, b


def _workspace(B, H, W, dev):
    return torch.empty(E.lib().rpcc_eval_workspace_bytes(B, H, W), dtype=torch.uint8, device=dev)


def nearest(p1, p2, bruteforce=False, visits=False, ws=None):
    """Exact nearest neighbours both ways (rpcc_eval_nn) for f32 [B,H,W,3] device clouds.
    -> dist1 f32 [B,P], idx1 i32 [B,P], dist2, idx2, n i32 [B,2], visits i32 [B,2,P] or None (first n entries valid)."""
    B, H, W = p1.shape[:3]
    P, dev = H * W, p1.device
    ws = _workspace(B, H, W, dev) if ws is None else ws
    d1 = torch.empty((B, P), dtype=torch.float32, device=dev)
    d2 = torch.empty_like(d1)
    i1 = torch.empty((B, P), dtype=torch.int32, device=dev)
    i2 = torch.empty_like(i1)
    n = torch.empty((B, 2), dtype=torch.int32, device=dev)
    vis = torch.zeros((B, 2, P), dtype=torch.int32, device=dev) if visits else None
    E.check(E.lib().rpcc_eval_nn(ptr(p1), ptr(p2), B, H, W, E.BRUTEFORCE if bruteforce else 0, ptr(d1), ptr(i1), ptr(d2), ptr(i2),
                                 ptr(n), ptr(vis), ptr(ws), stream()))
    return d1, i1, d2, i2, n, vis


def normals(p, r=59.7, bruteforce=False, neighbours=False, ws=None):
    """Oriented normals (rpcc_eval_normals) of f32 [B,H,W,3] device clouds -> (f64 [B,P,3], i32 [B,P,12] neighbour ranks or None)."""
    B, H, W = p.shape[:3]
    P, dev = H * W, p.device
    ws = _workspace(B, H, W, dev) if ws is None else ws
    nrm = torch.empty((B, P, 3), dtype=torch.float64, device=dev)
    nbr = torch.empty((B, P, E.KNN), dtype=torch.int32, device=dev) if neighbours else None
    E.check(E.lib().rpcc_eval_normals(ptr(p), B, H, W, float(r), E.BRUTEFORCE if bruteforce else 0, ptr(nrm), ptr(nbr), ptr(ws), stream()))
    return nrm, nbr


def frame_sums(p1, p2, nn12, nn21, normals1=None, f1_threshold=0.02, ws=None):
    """Per-frame fp64 sums (rpcc_eval_metrics) -> f64 [B,10]: n1, n2, sum sqrt(d) 1->2 / 2->1, sum d 1->2 / 2->1,
    count d < f1_threshold**2 1->2 / 2->1, point-to-plane sums 1->2 / 2->1."""
    B, H, W = p1.shape[:3]
    ws = _workspace(B, H, W, p1.device) if ws is None else ws
    s = torch.empty((B, E.NSUMS), dtype=torch.float64, device=p1.device)
    thr = float(np.float32(f1_threshold ** 2))   # fscore compares the float32 distances with the threshold as a float32
    E.check(E.lib().rpcc_eval_metrics(ptr(p1), ptr(p2), B, H, W, ptr(nn12), ptr(nn21), ptr(normals1), thr, ptr(s), ptr(ws), stream()))
    return s


def derive(s, r=59.7):
    """The metrics of the reference from frame_sums' [B,10] (fp64, on the sums' device) -> dict of [B] tensors."""
    n1, n2 = s[:, 0], s[:, 1]
    cd1, cd2 = s[:, 2] / n1, s[:, 3] / n2
    precision, recall = s[:, 6] / n1, s[:, 7] / n2
    f = 2 * precision * recall / (precision + recall)
    f = torch.where(precision + recall == 0, torch.zeros_like(f), f)   # fscore: a NaN from 0 / 0 becomes 0
    max_energy = 3 * r * r
    out = {"n1": n1, "n2": n2, "cd1": cd1, "cd2": cd2, "cd_mean": (cd1 + cd2) / 2, "f_score": f, "precision": precision, "recall": recall}
    for name, k in (("d1", 4), ("d2", 8)):
        m1, m2 = s[:, k] / n1, s[:, k + 1] / n2
        ps1, ps2 = 10 * torch.log10(max_energy / m1), 10 * torch.log10(max_energy / m2)
        out.update({name + "_mse_1": m1, name + "_mse_2": m2, name + "_psnr_1": ps1, name + "_psnr_2": ps2,
                    name + "_psnr": (ps1 + ps2) / 2})
    return out


def quality_batch(ri_orig, ri_rec, tm, f1_threshold=0.02, r=59.7, bruteforce=False):
    """All metrics of a batch: ri_orig / ri_rec f32 [B,H,W] device range images, tm f32 [H,W,3] device transform map.
    Points are ops.backproject's ri * tm.  -> dict of f64 [B] device tensors: cd1, cd2, cd_mean, f_score, precision, recall,
    d1_mse_1, d1_mse_2, d1_psnr, d2_mse_1, d2_mse_2, d2_psnr (and the per-side PSNRs and point counts).  A frame with an
    empty cloud on either side gets NaN.  Enqueued on the current stream; nothing synchronises."""
    B, H, W = ri_orig.shape
    if ri_rec.shape != ri_orig.shape or tuple(tm.shape) != (H, W, 3):
        raise ValueError("ri_orig / ri_rec must be [B,H,W] and tm [H,W,3] of the same H, W")
    p1 = ops.backproject(ri_orig.contiguous(), tm.contiguous())
    p2 = ops.backproject(ri_rec.contiguous(), tm.contiguous())
    ws = _workspace(B, H, W, p1.device)
    _, i1, _, i2, _, _ = nearest(p1, p2, bruteforce=bruteforce, ws=ws)
    nrm, _ = normals(p1, r, bruteforce=bruteforce, ws=ws)
    return derive(frame_sums(p1, p2, i1, i2, nrm, f1_threshold, ws=ws), r)


def psnr(x, max_energy):
    return 10 * np.log10(max_energy / x)


def calc_chamfer_distance(points1, points2, f1_threshold=0.02, out=True):
    """utils/evaluate_metrics.py:9-46: Chamfer distance and F-score of points2 against points1, same dict."""
    t = time.time()
    p1, p2 = _prepare(points1, points2)
    d1, i1, d2, i2, n, _ = nearest(p1, p2)
    m = derive(frame_sums(p1, p2, i1, i2, None, f1_threshold))
    n1, n2 = (int(v) for v in n[0].tolist())
    cd1, cd2 = float(m["cd1"][0]), float(m["cd2"][0])
    result = {
        "max": max(cd1, cd2),
        "mean": (cd1 + cd2) / 2,
        "sum": cd1 + cd2,
        "cd1": cd1,
        "cd2": cd2,
        "f_score": float(m["f_score"][0]),
        "precision": float(m["precision"][0]),
        "recall": float(m["recall"][0]),
        "chamfer_dist_info": {
            "dist1": d1[0, :n1].cpu().numpy(),
            "dist2": d2[0, :n2].cpu().numpy(),
            "idx1": i1[0, :n1].cpu().numpy(),
            "idx2": i2[0, :n2].cpu().numpy(),
        },
    }
    if out:
        for key, value in result.items():
            print(key, value)
        print("time cost: ", time.time() - t)
    return result


def _given_index(idx, n_len, n_range, name, P, dev):
    a = np.asarray(idx.cpu() if isinstance(idx, torch.Tensor) else idx).reshape(-1)
    if a.shape[0] != n_len:
        raise ValueError("%s holds %d entries, expected %d" % (name, a.shape[0], n_len))
    if a.size and (a.min() < 0 or a.max() >= n_range):
        raise ValueError("%s names a point outside 0 .. %d" % (name, n_range - 1))
    t = torch.zeros((1, P), dtype=torch.int32, device=dev)
    t[0, :n_len] = torch.from_numpy(a.astype(np.int32))
    return t


def calc_point_to_point_plane_psnr(points1, points2, idx1=None, idx2=None, r=59.7, out=True):
    """utils/evaluate_metrics.py:49-98: D1 (point-to-point) and D2 (point-to-plane) PSNR -> (point_to_point, point_to_plane)
    dicts.  As in the reference, idx1[j] is the nearest points1 point of points2[j] and idx2[i] the nearest points2 point of
    points1[i] (the Chamfer dict's idx2 / idx1); when not given they are searched."""
    t = time.time()
    p1, p2 = _prepare(points1, points2)
    P, dev = p1.shape[1] * p1.shape[2], p1.device
    ws = _workspace(1, p1.shape[1], p1.shape[2], dev)
    if idx1 is None or idx2 is None:
        _, c1, _, c2, n, _ = nearest(p1, p2, ws=ws)
    else:
        n = None
    if n is not None:
        n1, n2 = (int(v) for v in n[0].tolist())
    else:
        n1 = int(((p1[..., 0] + p1[..., 1]) + p1[..., 2] != 0).sum())
        n2 = int(((p2[..., 0] + p2[..., 1]) + p2[..., 2] != 0).sum())
    nn21 = c2 if idx1 is None else _given_index(idx1, n2, n1, "idx1", P, dev)
    nn12 = c1 if idx2 is None else _given_index(idx2, n1, n2, "idx2", P, dev)
    nrm, _ = normals(p1, r, ws=ws)
    m = derive(frame_sums(p1, p2, nn12, nn21, nrm, ws=ws), r)
    res = []
    for name in ("d1", "d2"):
        ps1, ps2 = float(m[name + "_psnr_1"][0]), float(m[name + "_psnr_2"][0])
        ms1, ms2 = float(m[name + "_mse_1"][0]), float(m[name + "_mse_2"][0])
        res.append({"psnr_1": ps1, "psnr_2": ps2, "mse_1": ms1, "mse_2": ms2, "psnr_mean": (ps1 + ps2) / 2, "mse_mean": (ms1 + ms2) / 2})
    if out:
        for title, d in zip(("point_to_point_result: ", "point_to_plane_result: "), res):
            print(title)
            for key, value in d.items():
                print(key, value)
        print("time cost: ", time.time() - t)
    return res[0], res[1]
