"""GPU: time of the inflate back-end (librpcc_inflate.so) on the containers of a 256-frame batch of the example sweep
(tests/golden/example_64E.npz: contour bits, index sequence, models and residuals, one copy per frame, uniform framework; 1024 gzip
members as deflate_codec writes them), and on one frame's four members: rpcc_inflate_decode with the members already in HBM, wall
clock from the launch to the stream's synchronize (after a warm-up, the median and the range of --reps runs); inflate_codec.decode_many
host to host (one copy each way around the launch); and -- labelled as a CPU number -- gzip.decompress on 16 threads over the same
members, which is how the host path decodes.  Every decoded byte is compared with gzip.decompress's before anything is timed.
Kernel time: run it under `rocprofv3 --kernel-trace --stats -d <dir> -- python tools_dev/inflate_time.py --reps 3 --no-host`.
Usage: python tools_dev/inflate_time.py [--frames 256] [--reps N] [--no-host] [--zlib] [--json FILE]"""
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
from rpcc_amd import deflate_codec, inflate_codec  # noqa: E402

THREADS = int(os.environ.get("OMP_NUM_THREADS", "16"))   # the CPU baseline: the cores this job may use, not the machine's


def frame_members(zlib_coded):
    import gen_golden_lz4
    a = gen_golden_lz4.arrays()
    per = [np.ascontiguousarray(a[k]).tobytes() for k in ("contour_map", "idx_sequence", "plane_param", "q_uniform")]
    return ([gzip.compress(p) for p in per] if zlib_coded else deflate_codec.compress_many(per)), per


def wall(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts)), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-host", dest="host", action="store_false", help="skip decode_many and the CPU part (kernel traces).")
    ap.add_argument("--zlib", action="store_true", help="members written by gzip.compress instead of deflate_codec.")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    members, plain = frame_members(args.zlib)
    assert [gzip.decompress(m) for m in members] == plain
    res = {"coder": "gzip.compress" if args.zlib else "deflate_codec", "member_bytes": [len(m) for m in members],
           "plain_bytes": [len(p) for p in plain]}
    for label, B in (("frame", 1), ("batch", args.frames)):
        blobs = members * B
        n = len(blobs)
        data = torch.from_numpy(np.frombuffer(b"".join(blobs), np.uint8).copy()).to(dev)
        lens = np.array([len(b) for b in blobs], np.int64)
        addr = data.data_ptr() + np.concatenate([[0], np.cumsum(lens)[:-1]])
        cap = np.array([len(p) for p in plain] * B, np.int64)
        off = np.concatenate([[0], np.cumsum(cap)[:-1]])
        meta = torch.from_numpy(np.stack([addr, lens, off, cap])).to(dev)
        dst = torch.empty(int(cap.sum()), dtype=torch.uint8, device=dev)
        state = {}

        def dec():
            state["out"] = inflate_codec.decode_descriptors(meta[0], meta[1], dst, meta[2], meta[3])
            torch.cuda.current_stream().synchronize()

        dec()
        assert not state["out"][1].any().item() and state["out"][0].cpu().numpy().tolist() == cap.tolist()
        assert dst.cpu().numpy().tobytes() == b"".join(plain) * B, "decoded bytes differ from gzip.decompress's"
        r = wall(dec, args.reps)
        r.update(streams=n, in_bytes=int(lens.sum()), out_bytes=int(cap.sum()), out_GBps=float(cap.sum()) / r["median_ms"] / 1e6)
        res["%s_device_resident" % label] = r
        if args.host:
            res["%s_decode_many" % label] = wall(lambda: inflate_codec.decode_many(blobs), max(3, args.reps // 4))
            with ThreadPoolExecutor(THREADS) as pool:
                list(pool.map(gzip.decompress, blobs[: 4 * THREADS]))
                ts = []
                for _ in range(max(3, args.reps // 4)):
                    t = time.perf_counter()
                    list(pool.map(gzip.decompress, blobs))
                    ts.append((time.perf_counter() - t) * 1e3)
            res["%s_cpu_gzip_decompress" % label] = {"threads": THREADS, "median_ms": float(np.median(ts)), "min_ms": float(min(ts)),
                                                     "max_ms": float(max(ts)), "reps": len(ts)}
    print(json.dumps(res))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
