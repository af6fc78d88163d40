"""GPU: frames per second of the decoding paths on the containers of 256 copies of the example sweep (tests/golden/example_64E.npz: 64 x 2000,
100 clusters, uniform framework), for each entropy back-end:
  (a) the chunked per-frame path of tools/decompress_datalist.py: BasicCompressor.decompress_dicts over 32 containers with the device decoder the
      back-end has (lz4_codec / device_entropy / device_bunzip2), then tools.decompress.decode_frame per frame;
  (b) the same with the host library's entropy decoder (bz2 / gzip; 'lz4' has no host decoder without the lz4 package: then (b) is (a));
  (c) pipeline.BatchDecompressor.decompress, host bytes in, NumPy arrays out;
  (d) BatchDecompressor.decompress_device with the containers uploaded before the clock starts, results left in HBM.
Wall clock from the call to a device synchronise, one warm-up run, then RUNS runs of each path in turn (a, b, c, d, a, b, ...): median (min - max).
(c)'s results are compared with (a)'s on the first chunk before anything is timed.  One process, one GPU.
Usage: python tools_dev/decode_times.py [--frames 256] [--runs 3]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rpcc_amd  # noqa: E402,F401
from rpcc_amd import pipeline  # noqa: E402
from rpcc_amd.compress_utils import BasicCompressor, unpack_bitstream  # noqa: E402
from rpcc_amd.dataset import build_dataset  # noqa: E402
from rpcc_amd.tools.decompress import decode_frame  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=256)
ap.add_argument("--runs", type=int, default=3)
args = ap.parse_args()

assert torch.cuda.is_available(), "decode_times.py measures on a GPU"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
xyz = np.load(os.path.join(ROOT, "tests", "golden", "example_64E.npz"))["xyz"]
T = build_dataset(lidar_type="Velodyne64E").PCTransformer
M, ACC, CHUNK, B = 100, 0.02, 32, args.frames
DEVICE_FLAGS = {"lz4": {}, "deflate": dict(device_entropy=True), "bzip2": dict(device_bunzip2=True)}


def per_frame(blobs, bc):
    out = []
    for c0 in range(0, len(blobs), CHUNK):
        cds = [unpack_bitstream(b) for b in blobs[c0: c0 + CHUNK]]
        for cd, d in zip(cds, bc.decompress_dicts(cds)):
            out.append(decode_frame(cd, bc, T, M, 2 * ACC, None, True, decoded=d))
    return out


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


print("| back-end | container bytes per frame | (a) per frame, device entropy | (b) per frame, host entropy | (c) BatchDecompressor.decompress | (d) decompress_device, resident |")
print("|---|---|---|---|---|---|")
for method in ("lz4", "deflate", "bzip2"):
    blobs = pipeline.BatchCompressor(T, cluster_num=M, accuracy=ACC, basic_compressor=method, seed=1).compress([xyz] * B, frame_ids=list(range(B)))
    bd = pipeline.BatchDecompressor(T, M, 2 * ACC, basic_compressor=method)
    dev_bc, host_bc = BasicCompressor(method_name=method, **DEVICE_FLAGS[method]), BasicCompressor(method_name=method)
    for got, ref in zip(bd.decompress(blobs[:CHUNK]), per_frame(blobs[:CHUNK], dev_bc)):
        assert all(np.array_equal(g.view(np.uint8), r.view(np.uint8)) for g, r in zip(got, ref)), method
    up = bd.upload(blobs)
    paths = [lambda: per_frame(blobs, dev_bc), lambda: per_frame(blobs, host_bc), lambda: bd.decompress(blobs),
             lambda: bd.decompress_device(blobs, uploaded=up)]
    for p in paths:
        clock(p)
    times = [[] for _ in paths]
    for _ in range(args.runs):
        for k, p in enumerate(paths):
            times[k].append(clock(p))
    cell = lambda t: "%.0f frames/s (%.0f - %.0f)" % (B / np.median(t), B / max(t), B / min(t))
    print("| %s | %d | %s |" % (method, sum(len(b) for b in blobs) // B, " | ".join(cell(t) for t in times)), flush=True)
