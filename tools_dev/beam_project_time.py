"""GPU: the projection through a per-beam elevation table against the even projection, on 256 copies of the example
sweep (tests/golden/example_64E.npz, 122 320 points, 64 x 2000) with the shipped table (lidar_cfg/Velodyne_HDL_64E_beams.csv):
  * rpcc_project_beams alone and rpcc_project (LDS-band path) alone, packed xyz;
  * the fused call with the table (rpcc_compress_batch_beams) and the even fused call (rpcc_compress_batch), cluster_num 100, uniform
    framework, point model, the ground fitted inside;
  * the share of points the table projection sends to the exact sequence (rpcc_project_beams_check).
Each time is the median of RUNS windows between device events, after a warm-up of every shape; a window holds as many calls as fill about
WINDOW_MS of device time (sized per variant from a first short window), and the two variants of a pair alternate window by window inside
one process.  The even numbers are those of THIS build: the even kernels' text is the same as before the table projection was added, and
that the same text gives the same times was checked once against a checkout of the commit before it (profiles/HISTORY.md).
Usage: python tools_dev/beam_project_time.py [--frames 256] [--json FILE]"""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rpcc_amd  # noqa: E402,F401
from rpcc_amd import ops  # noqa: E402
from rpcc_amd.transformer import PCTransformer  # noqa: E402

CFG = os.path.join(ROOT, "r-pcc_amd", "lidar_cfg")
RUNS, WINDOW_MS = 7, 300.0


def window_ms(fn, reps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def pair(a, b):
    """Medians (and min / max) of two variants whose windows alternate; -> [stats of a, stats of b]."""
    for _ in range(2):
        a(); b()
    reps = [max(20, int(math.ceil(WINDOW_MS / max(window_ms(f, 20), 1e-3)))) for f in (a, b)]
    ta, tb = [], []
    for _ in range(RUNS):
        ta.append(window_ms(a, reps[0]))
        tb.append(window_ms(b, reps[1]))
    return [dict(median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t), calls_per_window=r) for t, r in ((ta, reps[0]), (tb, reps[1]))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    yml = os.path.join(CFG, "Velodyne_HDL_64E.yaml")
    T, E = PCTransformer(yml, os.path.join(CFG, "Velodyne_HDL_64E_beams.csv")), PCTransformer(yml)
    one = np.ascontiguousarray(np.load(os.path.join(ROOT, "tests", "golden", "example_64E.npz"))["xyz"], dtype=np.float32)
    B, n = a.frames, one.shape[0]
    xyz = torch.from_numpy(one).to(dev).repeat(B, 1).contiguous()
    offs = torch.arange(B + 1, dtype=torch.int64, device=dev) * n
    P = T.H * T.W
    ri = torch.empty((B, T.H, T.W), dtype=torch.float32, device=dev)
    s_beams = torch.empty(ops._lib.lib().rpcc_project_beams_scratch_bytes(B * n, B, P), dtype=torch.uint8, device=dev)
    s_even = torch.empty(ops._lib.lib().rpcc_project_scratch_bytes(B * n, B, P), dtype=torch.uint8, device=dev)
    beams = T.beams_dev
    proj = pair(lambda: ops.project(xyz, offs, T.geom, ri=ri, scratch=s_beams, beams=beams),
                lambda: ops.project(xyz, offs, E.geom, ri=ri, scratch=s_even))
    buf_t, buf_e = (ops.BatchBuffers(B, T.geom, 100, dev, max_points=B * n) for _ in range(2))
    g_t, g_e = (torch.zeros((B, 4), dtype=torch.float64, device=dev) for _ in range(2))
    fid = list(range(B))
    fused = pair(lambda: ops.compress_batch(xyz, offs, T.tm_dev, g_t, buf_t, ground_seed=0, frame_ids=fid, beams=beams),
                 lambda: ops.compress_batch(xyz, offs, E.tm_dev, g_e, buf_e, ground_seed=0, frame_ids=fid))
    sure, bad, slow = ops.project_beams_check(torch.from_numpy(one).to(dev), T.geom, beams)
    out = dict(frames=B, points_per_frame=n, runs=RUNS, window_ms=WINDOW_MS,
               project_beams=proj[0], project_even=proj[1], fused_beams=fused[0], fused_even=fused[1],
               project_ratio=proj[0]["median_ms"] / proj[1]["median_ms"], fused_ratio=fused[0]["median_ms"] / fused[1]["median_ms"],
               frames_per_s=dict(project_beams=B / proj[0]["median_ms"] * 1e3, project_even=B / proj[1]["median_ms"] * 1e3,
                                 fused_beams=B / fused[0]["median_ms"] * 1e3, fused_even=B / fused[1]["median_ms"] * 1e3),
               exact_share=slow / n, fast_certain=sure, fast_disagree=bad)
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
