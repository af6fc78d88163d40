"""GPU: time of evaluate_metrics.quality_batch (Chamfer, F-score, D1 / D2 PSNR of a batch) on 64 synthetic 64 x 2048 sweeps and on the
example sweep replicated 64 times, each compressed and decoded at accuracy 0.02; pruned and brute-force searches (device events,
after a warm-up), tiles scanned per query, and -- labelled as a CPU number -- the scipy cKDTree search the reference's PSNR uses.
Kernel times: run it under `rocprofv3 --kernel-trace --stats -d <dir> -- python tools_dev/eval_metrics_time.py --reps 3`.
Usage: python tools_dev/eval_metrics_time.py [--reps N] [--json FILE]"""
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
from rpcc_amd import evaluate_metrics as em, ops, synth  # noqa: E402

B, ACC = 64, 0.02
THREADS = int(os.environ.get("OMP_NUM_THREADS", "16"))   # the CPU search: the cores this job may use, not the machine's


def roundtrip(frames, H, W, vmax_deg, vmin_deg, dev):
    args = (H, W, 2 * math.pi, math.radians(vmax_deg), math.radians(vmin_deg))
    geom, tm = ops.make_geom(*args), torch.from_numpy(ops.transform_map(*args)).to(dev)
    xyz = torch.cat([torch.as_tensor(np.asarray(f), dtype=torch.float32) for f in frames]).to(dev)
    offs = torch.tensor([0] + list(np.cumsum([len(f) for f in frames])), dtype=torch.int64, device=dev)
    buf = ops.BatchBuffers(len(frames), geom, 100, dev)
    ops.compress_batch(xyz, offs, tm, torch.zeros((len(frames), 4), dtype=torch.float64, device=dev), buf, ground_seed=1,
                       frame_ids=torch.arange(len(frames), device=dev), acc=2 * ACC)
    rec, _ = ops.decode(buf.seg, buf.q16, buf.model, tm, 2 * ACC)
    return buf.ri.clone(), rec, tm


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
    z = np.load(os.path.join(ROOT, "tests", "golden", "example_64E.npz"))
    sets = {
        "synth_64x2048": (64, 2048, 2.0, -24.9, [synth.make_frame(20000 + i, 64, 2048).numpy() for i in range(B)]),
        "example_64E_x64": (64, 2000, 2.0, -24.9, [z["xyz"]] * B),
    }
    rows = []
    for name, (H, W, vmax, vmin, frames) in sets.items():
        ri, rec, tm = roundtrip(frames, H, W, vmax, vmin, dev)
        row = {"set": name, "B": B, "H": H, "W": W, "accuracy": ACC}
        row["pruned_ms_per_batch"] = timed(lambda: em.quality_batch(ri, rec, tm), a.reps)
        row["brute_ms_per_batch"] = timed(lambda: em.quality_batch(ri, rec, tm, bruteforce=True), max(1, a.reps // 5))
        row["pruned_ms_per_frame"] = row["pruned_ms_per_batch"] / B
        row["brute_ms_per_frame"] = row["brute_ms_per_batch"] / B
        p1, p2 = ops.backproject(ri, tm), ops.backproject(rec, tm)
        row["nn_only_pruned_ms_per_batch"] = timed(lambda: em.nearest(p1, p2), a.reps)
        row["normals_only_pruned_ms_per_batch"] = timed(lambda: em.normals(p1), a.reps)
        _, _, _, _, n, vis = em.nearest(p1, p2, visits=True)
        n = n.cpu().numpy()
        v = vis.cpu().numpy()
        per_q = np.concatenate([v[b, d, :n[b, d]] for b in range(B) for d in range(2)])
        row["tiles_per_query_avg"] = float(per_q.mean())
        row["tiles_per_query_max"] = int(per_q.max())
        row["tiles_per_frame"] = ((H + 7) // 8) * ((W + 31) // 32)
        m = em.quality_batch(ri, rec, tm)
        row["frame0"] = {k: float(m[k][0]) for k in ("cd_mean", "f_score", "d1_psnr", "d2_psnr")}
        try:
            from scipy.spatial import cKDTree
            pc1 = p1[0].reshape(-1, 3).cpu().numpy()
            pc2 = p2[0].reshape(-1, 3).cpu().numpy()
            pc1, pc2 = pc1[pc1.sum(-1) != 0], pc2[pc2.sum(-1) != 0]
            t0 = time.time()
            cKDTree(pc1, balanced_tree=False).query(pc2, workers=THREADS)
            cKDTree(pc2, balanced_tree=False).query(pc1, workers=THREADS)
            row["cpu_ckdtree_both_directions_s_per_frame"] = time.time() - t0
        except ImportError:
            row["cpu_ckdtree_both_directions_s_per_frame"] = None
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
