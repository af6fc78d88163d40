"""GPU: tools/decompress_datalist.py --stream_decode against --batch_decode, .rpcc files in, .bin files out, on the containers of 256 copies
of the example sweep (tests/golden/example_64E.npz: 64 x 2000, 100 clusters, uniform framework) on local disk, the files in the page cache
(they are written just before), for 'rans' with rans_delta and for 'bzip2', with and without intensity.
  (a) tool, --batch_decode: tools.decompress_datalist.decompress(args) as the command line runs it, set-up included;
  (b) tool, --stream_decode: the same call with the flag (set-up included: the streams and the pinned buffers of the slots);
  (c) StreamingDecompressor.run on an object built before the clock starts: what a long datalist sees per 256 frames.
Wall clock from the call to the last file closed; one warm-up of each, then RUNS runs in turn (a, b, c, a, b, ...): median (min - max).  The
files of (b) and (c) are compared with (a)'s before anything is timed.  Also: the device time of the two rows launches for 256 frames (events
around rows.pack on decoded chunks of 32), and the bytes that cross the link per frame before and after.  One process, one GPU.
Usage: python tools_dev/decode_stream_time.py [--frames 256] [--runs 3] [--dir DIR]"""
import argparse
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rpcc_amd  # noqa: E402,F401
from rpcc_amd import loader, pipeline, rows  # noqa: E402
from rpcc_amd.dataset import build_dataset  # noqa: E402
from rpcc_amd.tools import decompress_datalist as tdl  # noqa: E402
from rpcc_amd.tools.compress import make_parser  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=256)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--dir", default=None, help="where the files go (default: a fresh directory under the system's temporary directory, removed at the end)")
args = ap.parse_args()

assert torch.cuda.is_available(), "decode_stream_time.py measures on a GPU"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
xyz = np.load(os.path.join(ROOT, "tests", "golden", "example_64E.npz"))["xyz"]
frame = np.ascontiguousarray(np.concatenate([xyz[:, :3], (np.random.default_rng(5).integers(0, 100, xyz.shape[0]) / np.float32(100))[:, None]], 1), np.float32)
LIDAR, M, ACC, B = "Velodyne64E", 100, 0.02, args.frames
T = build_dataset(lidar_type=LIDAR).PCTransformer
P = T.H * T.W
work = args.dir or tempfile.mkdtemp(prefix="decode_stream_")


def tree(root):
    return {os.path.relpath(os.path.join(d, f), root): open(os.path.join(d, f), "rb").read() for d, _, fs in os.walk(root) for f in fs}


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


cell = lambda t: "%.0f frames/s (%.0f - %.0f)" % (B / np.median(t), B / max(t), B / min(t))
print("| back-end | intensity | rows per frame | (a) tool --batch_decode | (b) tool --stream_decode | (c) StreamingDecompressor.run, object reused | "
      "rows launches, device time per %d frames | bytes over the link per frame: before -> after |" % B)
print("|---|---|---|---|---|---|---|---|")
try:
    for method, kw in (("rans", dict(rans_delta=True)), ("bzip2", {})):
        for intensity in (False, True):
            tag = "%s_%d" % (method, intensity)
            bc = pipeline.BatchCompressor(T, cluster_num=M, accuracy=ACC, basic_compressor=method, seed=1, intensity_scale=255.0 if intensity else None, **kw)
            blobs = bc.compress([frame if intensity else frame[:, :3]] * B, frame_ids=list(range(B)))
            src = os.path.join(work, tag, "in")
            os.makedirs(src, exist_ok=True)
            names = [os.path.join(src, "%06d.rpcc" % k) for k in range(B)]
            for n, b in zip(names, blobs):
                with open(n, "wb") as f:
                    f.write(b)
            lst = os.path.join(work, tag, "list.txt")
            with open(lst, "w") as f:
                f.write("\n".join(names) + "\n")
            flags = ["--datalist", lst, "--lidar", LIDAR, "--basic_compressor", method, "--cluster_num", str(M), "--accuracy", str(ACC)] + \
                    (["--intensity"] if intensity else []) + (["--rans_delta"] if kw else [])
            parse = lambda out, *more: make_parser(datalist=True).parse_args(flags + ["--output_dir", os.path.join(work, tag, out)] + list(more))
            a_batch, a_stream, a_run = parse("batch", "--batch_decode"), parse("stream", "--stream_decode"), parse("run")
            bd = pipeline.BatchDecompressor(T, M, 2 * ACC, basic_compressor=method, intensity=intensity)
            sd = loader.StreamingDecompressor(bd)
            outs = [tdl.output_path(a_run, n) for n in names]
            paths = [lambda: tdl.decompress(a_batch), lambda: tdl.decompress(a_stream), lambda: sd.run(names, outs)]
            for p in paths:     # warm-up, and the comparison
                clock(p)
            want = tree(os.path.join(work, tag, "batch"))
            assert len(want) == B and tree(os.path.join(work, tag, "stream")) == want and tree(os.path.join(work, tag, "run")) == want, tag
            times = [[] for _ in paths]
            for _ in range(args.runs):
                for k, p in enumerate(paths):
                    times[k].append(clock(p))
            # the two launches alone: a decoded chunk on the device, packed B / chunk times between two events
            n = min(bd.chunk, B)
            images = bd.rows_buffers(n)
            bd._chunk_device(blobs[:n], images)
            out_rows = torch.empty((n * P, 4), dtype=torch.float32, device=bd.device)
            pack = lambda: rows.pack(images[3], images[4] if intensity else None, images[2], rows=out_rows)
            pack()
            torch.cuda.synchronize()
            dev_ms = []
            for _ in range(args.runs):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(-(-B // n)):
                    pack()
                e1.record()
                e1.synchronize()
                dev_ms.append(e0.elapsed_time(e1))
            kept = len(next(iter(want.values()))) // 16
            before = P * (images[1].element_size() + 4 + 12 + (4 if intensity else 0)) + 4
            after = 16 * kept + 4 + 8 + 4
            print("| %s | %s | %d | %s | %s | %s | %.3f ms (%.3f - %.3f) | %d -> %d |" % (
                method + (" + rans_delta" if kw else ""), "yes" if intensity else "no", kept, cell(times[0]), cell(times[1]), cell(times[2]),
                np.median(dev_ms), min(dev_ms), max(dev_ms), before, after), flush=True)
            del sd, bd, images, out_rows
finally:
    if args.dir is None:
        shutil.rmtree(work, ignore_errors=True)
