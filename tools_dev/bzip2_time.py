"""GPU: time of the bzip2 encoder (librpcc_bzip2.so) on the example sweep's four arrays (tests/golden/example_64E.npz: contour bits,
index sequence, models, residuals): rpcc_bzip2_encode over 4 streams and over 256 copies of them (1024 streams), inputs already in HBM
(device events, after a warm-up, minimum / median / maximum over the repetitions); compress_many host to host (wall clock); -- labelled
as a CPU number -- bz2.compress on 16 threads over the same arrays, which is how 'bzip2' is coded without device_bzip2; and
BatchCompressor end to end (three batches in flight, wall clock) with the flag and with the host pool.
Kernel times: run it under `rocprofv3 --kernel-trace --stats -d <dir> -- python tools_dev/bzip2_time.py --reps 3 --no-batch`.
Usage: python tools_dev/bzip2_time.py [--frames 256] [--reps N] [--no-batch] [--json FILE]"""
import argparse
import bz2
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rpcc_amd  # noqa: E402,F401
from rpcc_amd import bzip2_codec  # noqa: E402

THREADS = int(os.environ.get("OMP_NUM_THREADS", "16"))   # the CPU baseline: the cores this job may use, not the machine's


def spread(fn, reps):
    """-> (min, median, max) ms of fn over reps runs, each between two events, after one warm-up."""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return [float(np.min(ms)), float(np.median(ms)), float(np.max(ms))]


def wall(fn, reps):
    fn()
    ms = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t) * 1e3)
    return [float(np.min(ms)), float(np.median(ms)), float(np.max(ms))]


def frame_arrays():
    import bzip2_cases
    return list(bzip2_cases.golden_arrays().values())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-batch", dest="batch", action="store_false", help="skip the BatchCompressor and CPU parts (kernel traces).")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    per = frame_arrays()
    res = {"frames": args.frames, "bytes_per_frame": sum(len(a) for a in per), "reps": args.reps, "ms": "min / median / max"}
    for label, B in (("4_streams", 1), ("%d_streams" % (4 * args.frames), args.frames)):
        arrays = per * B
        data = torch.from_numpy(np.frombuffer(b"".join(arrays), np.uint8).copy()).to(dev)
        offs = np.concatenate([[0], np.cumsum([len(a) for a in arrays])[:-1]])
        desc = torch.tensor([[data.data_ptr() + int(o) for o in offs], [len(a) for a in arrays]], dtype=torch.int64, device=dev)
        caps = [len(a) for a in arrays]
        ws = torch.empty(bzip2_codec.workspace_bytes(len(arrays), sum(caps)) // 8 + 2, dtype=torch.int64, device=dev)
        ws = ws[(-ws.data_ptr() // 8) % 2:]
        state = {}

        def enc():
            state["out"] = bzip2_codec.encode_descriptors(desc[0], desc[1], caps, ws=ws)

        res["encode_%s_ms" % label] = spread(enc, args.reps)
        slots, _, dst_len, off = state["out"]
        got, h = dst_len.cpu().numpy(), slots.cpu().numpy()
        assert (got > 0).all()
        for k in range(len(per)):        # the last frame's streams decode to the arrays
            j = len(arrays) - len(per) + k
            assert bz2.decompress(h[off[j]: off[j] + got[j]].tobytes()) == per[k], "bz2.decompress does not return the array"
        res["compressed_bytes_per_frame"] = int(got[-len(per):].sum()) + 4 * len(per)
        res["compress_many_%s_ms" % label] = wall(lambda: bzip2_codec.compress_many(arrays), max(2, args.reps // 2))

    if args.batch:
        arrays = per * args.frames
        with ThreadPoolExecutor(THREADS) as pool:
            res["cpu_bz2_threads"] = THREADS
            res["cpu_bz2_%d_streams_ms" % len(arrays)] = wall(lambda: list(pool.map(bz2.compress, arrays)), max(2, args.reps // 2))
            res["cpu_bz2_4_streams_ms"] = wall(lambda: list(pool.map(bz2.compress, per)), args.reps)
            res["cpu_bz2_compressed_bytes_per_frame"] = sum(len(bz2.compress(a)) for a in per) + 4 * len(per)
        # BatchCompressor end to end, three batches in flight; the host coder runs on the pool, as the datalist tool runs it
        from oracle import oracle as orc
        from rpcc_amd import dataset, synth
        from rpcc_amd.pipeline import BatchCompressor
        gd = orc.GEOMS["Velodyne64E_2048"]
        T = dataset.build_dataset(lidar_type="Velodyne64E_2048").PCTransformer
        nb = min(args.frames, 64)
        frames = [synth.make_frame(5000 + i, gd["H"], gd["W"], vmax_deg=gd["vmax_deg"], vmin_deg=gd["vmin_deg"]).numpy() for i in range(nb)]
        with ThreadPoolExecutor(THREADS) as pool:
            for label, flag in (("bzip2_device", True), ("bzip2_host", False)):
                bc = BatchCompressor(T, basic_compressor="bzip2", seed=1, device_bzip2=flag)
                bc.collect(bc.submit(frames), pool=pool)   # warm-up
                torch.cuda.synchronize()
                t = time.perf_counter()
                ctxs = [bc.submit(frames) for _ in range(3)]
                got = [bc.collect(c, pool=pool) for c in ctxs]
                dt = time.perf_counter() - t
                res["batch_%s_frames_per_s" % label] = 3 * nb / dt
                res["batch_%s_bytes_per_frame" % label] = float(np.mean([len(b) for b in got[0]]))
            one = frames[:1]
            for label, flag in (("bzip2_device", True), ("bzip2_host", False)):
                bc = BatchCompressor(T, basic_compressor="bzip2", seed=1, device_bzip2=flag)
                res["one_frame_%s_ms" % label] = wall(lambda: bc.compress(one), args.reps)
    print(json.dumps(res))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
