"""GPU: time of the deflate back-end (librpcc_deflate.so) on a 256-frame batch of 64 x 2048-class arrays: encode + container
compaction (device events, after a warm-up, inputs already in HBM), beside the LZ4 back-end's encode + compaction over the same
arrays in the same process; BatchCompressor end to end (three batches in flight, wall clock) with 'deflate' on the device,
'deflate' on the host pool, 'lz4' and 'bzip2'; and -- labelled as a CPU number -- gzip.compress on 16 threads over the same
arrays.  The arrays are the example sweep's (tests/golden/example_64E.npz): contour bits, index sequence, models and residuals,
one copy per frame, uniform framework.
Kernel times: run it under `rocprofv3 --kernel-trace --stats -d <dir> -- python tools_dev/deflate_time.py --reps 3 --no-batch`.
Usage: python tools_dev/deflate_time.py [--frames 256] [--reps N] [--no-batch] [--json FILE]"""
import argparse
import gzip
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import rpcc_amd  # noqa: E402,F401
from rpcc_amd import deflate_codec, lz4_codec  # noqa: E402

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


def frame_arrays():
    import gen_golden_lz4
    a = gen_golden_lz4.arrays()
    return [a["contour_map"], a["idx_sequence"], a["plane_param"], a["q_uniform"]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-batch", dest="batch", action="store_false", help="skip the BatchCompressor and CPU parts (kernel traces).")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B = args.frames
    per = frame_arrays()
    k = len(per)
    arrays = per * B
    nbytes = sum(len(a) for a in arrays)
    data = torch.from_numpy(np.frombuffer(b"".join(arrays), np.uint8).copy()).to(dev)
    offs = np.concatenate([[0], np.cumsum([len(a) for a in arrays])[:-1]])
    desc = torch.tensor([[data.data_ptr() + int(o) for o in offs], [len(a) for a in arrays]], dtype=torch.int64, device=dev)
    caps = [len(a) for a in arrays]
    res = {"frames": B, "bytes_per_frame": nbytes // B, "streams": len(arrays)}

    for name, codec, host in (("deflate", deflate_codec, deflate_codec.compress_many), ("lz4", lz4_codec, lz4_codec.dumps_many)):
        state = {}

        def enc():
            slots, dst_off, dst_len, _ = codec.encode_descriptors(desc[0], desc[1], caps)
            out, frame = lz4_codec.pack_containers(slots, dst_off, dst_len, B, k, slots.numel() + 4 * len(arrays))
            state.update(out=out, frame=frame)

        ms = timed(enc, args.reps)
        res["%s_encode_pack_ms" % name] = ms
        res["%s_encode_pack_GBps" % name] = nbytes / ms / 1e6
        res["%s_encode_pack_frames_per_s" % name] = B / ms * 1e3
        # the containers equal the list encoder's streams (a spot check on the last frame of the batch)
        fr = state["frame"].cpu().numpy()
        blob = state["out"][int(fr[0, -1]): int(fr[0, -1] + fr[1, -1])].cpu().numpy().tobytes()
        parts = host(per)
        assert blob == b"".join(len(b).to_bytes(4, "little") + b for b in parts), "container mismatch"
        if name == "deflate":
            assert [gzip.decompress(b) for b in parts] == per, "gzip.decompress does not return the arrays"
        res["%s_compressed_bytes_per_frame" % name] = int(fr[1, -1])

    if args.batch:
        # BatchCompressor end to end, three batches in flight; the host coders run on the pool, as the datalist tool runs them
        from oracle import oracle as orc
        from rpcc_amd import dataset, synth
        from rpcc_amd.pipeline import BatchCompressor
        gd = orc.GEOMS["Velodyne64E_2048"]
        T = dataset.build_dataset(lidar_type="Velodyne64E_2048").PCTransformer
        nb = min(B, 64)
        frames = [synth.make_frame(5000 + i, gd["H"], gd["W"], vmax_deg=gd["vmax_deg"], vmin_deg=gd["vmin_deg"]).numpy() for i in range(nb)]
        with ThreadPoolExecutor(THREADS) as pool:
            for label, m, dev_entropy in (("deflate_device", "deflate", True), ("deflate_host", "deflate", False), ("lz4", "lz4", False),
                                          ("bzip2", "bzip2", False)):
                bc = BatchCompressor(T, basic_compressor=m, seed=1, device_entropy=dev_entropy)
                bc.collect(bc.submit(frames), pool=pool)   # warm-up
                torch.cuda.synchronize()
                t = time.perf_counter()
                ctxs = [bc.submit(frames) for _ in range(3)]
                got = [bc.collect(c, pool=pool) for c in ctxs]
                dt = time.perf_counter() - t
                res["batch_%s_frames_per_s" % label] = 3 * nb / dt
                res["batch_%s_bytes_per_frame" % label] = float(np.mean([len(b) for b in got[0]]))

        with ThreadPoolExecutor(THREADS) as pool:
            list(pool.map(gzip.compress, arrays[: 4 * THREADS]))
            t = time.perf_counter()
            sizes = list(pool.map(lambda a: len(gzip.compress(a)), arrays))
            dt = time.perf_counter() - t
        res["cpu_gzip_threads"] = THREADS
        res["cpu_gzip_ms"] = dt * 1e3
        res["cpu_gzip_GBps"] = nbytes / dt / 1e9
        res["cpu_gzip_frames_per_s"] = B / dt
        res["cpu_gzip_compressed_bytes_per_frame"] = sum(sizes[:k]) + 4 * k
    print(json.dumps(res))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
