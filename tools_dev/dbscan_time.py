"""GPU: time of rpcc_amd.dbscan.dbscan_segment (DBSCAN, eps 1.5, min_points 10) on synthetic 64 x 2048 sweeps at B = 1 and
B = 32, pruned against brute force (device events, after a warm-up), pair tests and tiles visited per frame, and --
labelled as a CPU number -- sklearn's DBSCAN on frame 0 when sklearn is installed.
Kernel times: run it under `rocprofv3 --kernel-trace --stats -d <dir> -- python tools_dev/dbscan_time.py --reps 3`.
Usage: python tools_dev/dbscan_time.py [--reps N] [--json FILE]"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rpcc_amd  # noqa: E402,F401
from rpcc_amd import ops, synth  # noqa: E402
from rpcc_amd.dbscan import dbscan_segment  # noqa: E402

H, W, VMAX, VMIN, EPS = 64, 2048, 2.0, -24.9, 1.5
THREADS = int(os.environ.get("OMP_NUM_THREADS", "16"))   # the CPU baseline: the cores this job may use, not the machine's


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    args = (H, W, 2 * math.pi, math.radians(VMAX), math.radians(VMIN))
    geom, tm = ops.make_geom(*args), torch.from_numpy(ops.transform_map(*args)).to(dev)
    frames = [synth.make_frame(30000 + i, H, W, vmax_deg=VMAX, vmin_deg=VMIN) for i in range(32)]
    xyz = torch.cat(frames).to(dev)
    offs = torch.tensor([0] + list(np.cumsum([len(f) for f in frames])), dtype=torch.int64, device=dev)
    ri_all = ops.project(xyz, offs, geom)
    ground_all, _ = ops.ground_ransac(ri_all, tm, seed=1)
    rows = []
    for B in (1, 32):
        ri, ground = ri_all[:B].contiguous(), ground_all[:B].contiguous()
        row = {"B": B, "H": H, "W": W, "eps": EPS, "min_points": 10}
        row["pruned_ms_per_frame"] = timed(lambda: dbscan_segment(ri, tm, ground, EPS), a.reps) / B
        row["brute_ms_per_frame"] = timed(lambda: dbscan_segment(ri, tm, ground, EPS, brute_force=True), max(1, a.reps // 5)) / B
        seg, mx, st = dbscan_segment(ri, tm, ground, EPS, stats=True)
        _, _, bst = dbscan_segment(ri, tm, ground, EPS, brute_force=True, stats=True)
        st, bst = st.cpu().numpy(), bst.cpu().numpy()
        row["pair_tests_per_frame_pruned"] = float(st[:, 0].mean())
        row["pair_tests_per_frame_brute"] = float(bst[:, 0].mean())
        row["tiles_visited_per_frame_pruned"] = float(st[:, 1].mean())
        row["tiles_visited_per_frame_brute"] = float(bst[:, 1].mean())
        row["max_label_frame0"] = int(mx[0])
        s0 = seg[0].cpu().numpy()
        row["nonground_points_frame0"] = int((s0 >= 2).sum() + ((s0 == 1) & (ri[0].cpu().numpy() == 0)).sum())
        rows.append(row)
        print(json.dumps(row), flush=True)
    try:
        from sklearn.cluster import DBSCAN
    except ImportError:
        DBSCAN = None
    if DBSCAN is not None:
        r0, t0_, g0 = ri_all[0].cpu().numpy(), tm.cpu().numpy(), ground_all[0].cpu().numpy()
        den = (g0[0] * t0_[..., 0].astype(np.float64) + g0[1] * t0_[..., 1]) + g0[2] * t0_[..., 2]
        with np.errstate(divide="ignore", invalid="ignore"):
            ng = np.abs(r0.astype(np.float64) - (-g0[3] / den)) > 0.5
        pts = (r0[..., None] * t0_)[ng].astype(np.float64)
        t = time.time()
        DBSCAN(eps=EPS, min_samples=10, n_jobs=THREADS).fit(pts)
        row = {"cpu_sklearn_dbscan_s_per_frame": time.time() - t, "points": int(pts.shape[0]), "n_jobs": THREADS}
    else:
        row = {"cpu_sklearn_dbscan_s_per_frame": None}
    rows.append(row)
    print(json.dumps(row), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
