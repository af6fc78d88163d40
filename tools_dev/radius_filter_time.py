"""GPU: radius outlier removal (outlier.radius_outlier_mask, librpcc_filter.so) on the example sweep
(tests/golden/example_64E.npz, 122 320 points, nb_points 3, radius 1.0), replicated to B = 1 and B = 32 frames.  Per B, each the median of
3 timings (device events around REPS back-to-back calls, after a warm-up of every shape):
  * pruned search, stored order;
  * RPCC_FILTER_BRUTEFORCE (every pair in fp64);
  * pruned search, every frame's list shuffled;
  * pair tests and tiles visited per frame from stats (stored and shuffled);
  * the device part of a pipeline.BatchCompressor step (FPS, compress_device) without and with radius_outlier_removal=(3, 1.0), and the
    filter's share of the step with it (the filter alone over the step).
Where scipy is present: cKDTree.query_ball_point(return_length=True) of one sweep on the job's CPUs, a CPU figure for scale.
Usage: python tools_dev/radius_filter_time.py [--batches 1 32] [--json FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rpcc_amd  # noqa: E402,F401
from rpcc_amd.dataset import build_dataset  # noqa: E402
from rpcc_amd.outlier import radius_outlier_mask, workspace_bytes  # noqa: E402
from rpcc_amd.pipeline import BatchCompressor  # noqa: E402

NB_POINTS, RADIUS, RUNS = 3, 1.0, 3
THREADS = int(os.environ.get("OMP_NUM_THREADS", "16"))   # the CPUs this job may use, not the machine's


def device_ms(fn, reps):
    """reps back-to-back fn() on the current stream between two events -> milliseconds per call (the stream is drained before and after)."""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def median_ms(fn, reps):
    fn()                                   # warm-up of this shape
    return round(statistics.median(device_ms(fn, reps) for _ in range(RUNS)), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 32])
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    dev = torch.device("cuda:0")
    sweep = np.load(os.path.join(ROOT, "tests", "golden", "example_64E.npz"))["xyz"].astype(np.float32)
    n = sweep.shape[0]
    T = build_dataset(lidar_type="Velodyne64E").PCTransformer
    out = dict(points=n, nb_points=NB_POINTS, radius=RADIUS, runs=RUNS, threads=THREADS, batches={})
    for B in a.batches:
        rng = np.random.default_rng(B)
        stored = torch.from_numpy(np.tile(sweep, (B, 1))).to(dev)
        shuffled = torch.from_numpy(np.concatenate([sweep[rng.permutation(n)] for _ in range(B)])).to(dev)
        offsets = torch.arange(B + 1, dtype=torch.int64, device=dev) * n
        ws = torch.empty(workspace_bytes(B * n, B), dtype=torch.uint8, device=dev)
        call = lambda xyz, brute=False, **kw: radius_outlier_mask(xyz, offsets, NB_POINTS, RADIUS, brute_force=brute, ws=ws, **kw)
        r = dict(frames=B)
        ref = call(stored, stats=True)
        bru = call(stored, brute=True, stats=True)
        shf = call(shuffled, stats=True)
        torch.cuda.synchronize()
        assert torch.equal(ref.keep, bru.keep) and torch.equal(ref.count, bru.count)
        assert int(ref.kept[0]) == int(shf.kept[0])
        r["removed_per_frame"] = n - int(ref.kept[0])
        r["pruned_stored_ms"] = median_ms(lambda: call(stored, masked=True), 100 if B == 1 else 5)
        r["bruteforce_ms"] = median_ms(lambda: call(stored, brute=True, masked=True), 3 if B == 1 else 1)
        r["pruned_shuffled_ms"] = median_ms(lambda: call(shuffled, masked=True), 5 if B == 1 else 1)
        r["pruned_not_slower_than_bruteforce"] = bool(r["pruned_stored_ms"] <= r["bruteforce_ms"])
        for name, s in (("stored", ref.stats), ("shuffled", shf.stats), ("bruteforce", bru.stats)):
            r["pair_tests_per_frame_" + name] = int(s[:, 0].sum()) // B
            r["tiles_visited_per_frame_" + name] = int(s[:, 1].sum()) // B
        ground = torch.tensor([[0.0, 0.0, 1.0, 1.7]] * B, dtype=torch.float64, device=dev)
        ids = list(range(B))
        plain = BatchCompressor(T, accuracy=0.02, seed=1)
        filt = BatchCompressor(T, accuracy=0.02, seed=1, radius_outlier_removal=(NB_POINTS, RADIUS))
        r["step_plain_ms"] = median_ms(lambda: plain.compress_device(stored, offsets, ground, ids), 3)
        r["step_filtered_ms"] = median_ms(lambda: filt.compress_device(stored, offsets, ground, ids), 3)
        r["filter_share_of_filtered_step"] = round(r["pruned_stored_ms"] / r["step_filtered_ms"], 4)
        out["batches"][str(B)] = r
        del stored, shuffled, ws
    try:
        from scipy.spatial import cKDTree
        p = sweep.astype(np.float64)

        def tree():
            t0 = time.perf_counter()
            cKDTree(p).query_ball_point(p, RADIUS, return_length=True, workers=THREADS)
            return 1e3 * (time.perf_counter() - t0)
        tree()
        out["ckdtree_cpu_ms_per_frame"] = round(statistics.median(tree() for _ in range(RUNS)), 1)
    except ImportError:
        out["ckdtree_cpu_ms_per_frame"] = None
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
