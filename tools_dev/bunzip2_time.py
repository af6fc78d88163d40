"""GPU: time of the bunzip2 back-end (librpcc_bunzip2.so) on the containers of a 256-frame batch of the example sweep
(tests/golden/example_64E.npz 'rpcc': contour bits, index sequence, models and residuals as bz2.compress wrote them, one copy per frame;
1024 bzip2 streams), and on one frame's four streams: rpcc_bunzip2_decode with the streams already in HBM, wall clock from the launch to
the stream's synchronize (after a warm-up, the median and the range of --reps runs); bunzip2_codec.decode_many host to host (one copy
each way around the launch); and -- labelled as a CPU number -- bz2.decompress on 16 threads over the same streams, which is how the host
path decodes.  Every decoded byte is compared with bz2.decompress's before anything is timed.
--build-serial-walk FILE compiles (no GPU needed) a library whose walk is one sublist per stream -- one dependent load per byte -- and
--lib FILE times that library instead: the comparison that says what the sublists are worth.  A developer option, not an ABI flag.
Kernel time: run it under `rocprofv3 --kernel-trace --stats -d <dir> -- python tools_dev/bunzip2_time.py --reps 3 --no-host`.
Usage: python tools_dev/bunzip2_time.py [--frames 256] [--reps N] [--no-host] [--lib FILE] [--json FILE]"""
import argparse
import bz2
import json
import os
import struct
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

THREADS = int(os.environ.get("OMP_NUM_THREADS", "16"))   # the CPU baseline: the cores this job may use, not the machine's


def frame_members():
    blob = np.load(os.path.join(ROOT, "tests", "golden", "example_64E.npz"))["rpcc"].tobytes()
    out, off = [], 0
    while off < len(blob):
        (n,) = struct.unpack_from("i", blob, off)
        out.append(blob[off + 4: off + 4 + n])
        off += 4 + n
    return out


def wall(fn, reps, sync):
    fn()
    sync()
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
    ap.add_argument("--lib", default=None, help="time this build of librpcc_bunzip2.so (RPCC_BUNZIP2_LIB).")
    ap.add_argument("--build-serial-walk", dest="build_serial", default=None, metavar="FILE",
                    help="compile the library with -DBZ_SERIAL_WALK into FILE and exit.")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if args.build_serial:
        import rpcc_amd  # noqa: F401
        from rpcc_amd import build as b
        subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + b.HIPCC_FLAGS + ["-DBZ_SERIAL_WALK", b.BUNZIP2_SRC, "-o", args.build_serial])
        print(args.build_serial)
        return
    if args.lib:
        os.environ["RPCC_BUNZIP2_LIB"] = os.path.abspath(args.lib)
    import torch
    import rpcc_amd  # noqa: F401
    from rpcc_amd import bunzip2_codec
    dev = torch.device("cuda:0")
    members = frame_members()
    plain = [bz2.decompress(m) for m in members]
    res = {"library": args.lib or "librpcc_bunzip2.so", "member_bytes": [len(m) for m in members], "plain_bytes": [len(p) for p in plain]}
    for label, B in (("frame", 1), ("batch", args.frames)):
        blobs = members * B
        n = len(blobs)
        data = torch.from_numpy(np.frombuffer(b"".join(blobs), np.uint8).copy()).to(dev)
        lens = np.array([len(b) for b in blobs], np.int64)
        addr = data.data_ptr() + np.concatenate([[0], np.cumsum(lens)[:-1]])
        cap = np.array([len(p) for p in plain] * B, np.int64)
        off = np.concatenate([[0], np.cumsum(cap)[:-1]])
        wcap = np.array([bunzip2_codec.work_bytes(bunzip2_codec.block_bound(int(b[3:4]), c)) for b, c in zip(blobs, cap)], np.int64)
        woff = np.concatenate([[0], np.cumsum((wcap + 7) // 8 * 8)[:-1]])
        meta = torch.from_numpy(np.stack([addr, lens, off, cap, woff, wcap])).to(dev)
        dst = torch.empty(int(cap.sum()), dtype=torch.uint8, device=dev)
        work = torch.empty(int(woff[-1] + wcap[-1]), dtype=torch.uint8, device=dev)
        state = {}

        def dec():
            state["out"] = bunzip2_codec.decode_descriptors(meta[0], meta[1], dst, meta[2], meta[3], work, meta[4], meta[5])
            torch.cuda.current_stream().synchronize()

        dec()
        assert not state["out"][2].any().item() and state["out"][0].cpu().numpy().tolist() == cap.tolist()
        assert state["out"][1].cpu().numpy().tolist() == lens.tolist()
        assert dst.cpu().numpy().tobytes() == b"".join(plain) * B, "decoded bytes differ from bz2.decompress's"
        r = wall(dec, args.reps, torch.cuda.synchronize)
        r.update(streams=n, in_bytes=int(lens.sum()), out_bytes=int(cap.sum()), work_bytes=int(work.numel()),
                 out_GBps=float(cap.sum()) / r["median_ms"] / 1e6)
        res["%s_device_resident" % label] = r
        if args.host:
            assert bunzip2_codec.decode_many(blobs)[1] == plain * B
            res["%s_decode_many" % label] = wall(lambda: bunzip2_codec.decode_many(blobs), max(3, args.reps // 4), torch.cuda.synchronize)
            with ThreadPoolExecutor(THREADS) as pool:
                list(pool.map(bz2.decompress, blobs[: 4 * THREADS]))
                ts = []
                for _ in range(max(3, args.reps // 4)):
                    t = time.perf_counter()
                    list(pool.map(bz2.decompress, blobs))
                    ts.append((time.perf_counter() - t) * 1e3)
            res["%s_cpu_bz2_decompress" % label] = {"threads": THREADS, "median_ms": float(np.median(ts)), "min_ms": float(min(ts)),
                                                    "max_ms": float(max(ts)), "reps": len(ts)}
    print(json.dumps(res))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
