"""GPU: basic_compressor 'rans', without and with rans_delta (the delta filter on the int16 residuals, format version 2), beside 'lz4' (the
fastest of the other device back-ends in every row, and untouched by the rans work), in one process on one GPU.  Inputs as in tools_dev/codec_times.py and tools_dev/decode_times.py: the four payload arrays and the containers of 256
copies of the example sweep (tests/golden/example_64E.npz: 64 x 2000, 100 clusters, uniform framework) -- 1024 streams.
  1. encode and decode of the 1024 streams with everything resident in HBM (encode_tensors; decode_descriptors into a buffer made before);
  2. compress_many / decompress_many (lz4: dumps_many / loads_many), host bytes in, host bytes out;
  3. BatchCompressor and BatchDecompressor, frames/s, host to host and resident (points / containers uploaded before the clock starts);
  4. one frame's four streams alone, resident, beside bz2 and zlib on the host for the same four arrays;
  5. container bytes of the example sweep under lz4, deflate, bzip2 and rans without and with the filter at chunk_log2 14 / 15 / 16.
Wall clock from the call to a device synchronise, one warm-up, then RUNS runs with the back-ends taking turns: median (min - max).
Usage: python tools_dev/rans_times.py [--frames 256] [--runs 3]"""
import argparse
import bz2
import os
import sys
import time
import zlib

import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rpcc_amd  # noqa: E402,F401
from rpcc_amd import entropy, lz4_codec, pipeline, rans_codec  # noqa: E402
from rpcc_amd.compress_utils import BasicCompressor, unpack_bitstream  # noqa: E402
from rpcc_amd.dataset import build_dataset  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=256)
ap.add_argument("--runs", type=int, default=3)
args = ap.parse_args()

assert torch.cuda.is_available(), "rans_times.py measures on a GPU"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
xyz = np.load(os.path.join(ROOT, "tests", "golden", "example_64E.npz"))["xyz"]
T = build_dataset(lidar_type="Velodyne64E").PCTransformer
dev = T.device
M, ACC, B = 100, 0.02, args.frames
DTYPES = {"contour_map": np.uint8, "idx_sequence": np.uint16, "plane_param": np.float32, "residual_quantized": np.int16}


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def measure(paths):
    """paths: {name: callable} -> {name: [seconds] * RUNS}, the paths taking turns after one warm-up each."""
    for p in paths.values():
        clock(p)
    times = {k: [] for k in paths}
    for _ in range(args.runs):
        for k, p in paths.items():
            times[k].append(clock(p))
    return times


def ms(t):
    return "%.2f ms (%.2f - %.2f)" % (1e3 * np.median(t), 1e3 * min(t), 1e3 * max(t))


def fps(t):
    return "%.0f frames/s (%.0f - %.0f)" % (B / np.median(t), B / max(t), B / min(t))


blob = pipeline.BatchCompressor(T, cluster_num=M, accuracy=ACC, basic_compressor="bzip2", seed=1).compress([xyz], frame_ids=[0])[0]
frame = [np.frombuffer(bz2.decompress(v), DTYPES[k]) for k, v in unpack_bitstream(blob).items()]
arrays = frame * B
raw = sum(a.nbytes for a in frame)
print("one frame: %d streams, %d bytes (%s); %d streams in all" % (len(frame), raw, ", ".join("%s %d" % (k, a.nbytes) for k, a in zip(DTYPES, frame)), len(arrays)))
# 'rans delta': rans_codec with the filter where its rule gives one (the arrays' dtypes: the tensors below are made from them)
_NP = {torch.uint8: np.uint8, torch.int16: np.int16, torch.uint16: np.uint16, torch.float32: np.float32}
rans_delta = types.SimpleNamespace(
    encode_tensors=lambda ts: rans_codec.encode_tensors(ts, filters=[rans_codec.delta_filter(_NP[t.dtype]) for t in ts]),
    decode_descriptors=rans_codec.decode_descriptors)
CODECS = {"rans": (rans_codec, rans_codec.compress_many, rans_codec.decompress_many),
          "rans delta": (rans_delta, rans_codec.compress_many_delta, rans_codec.decompress_many),
          "lz4": (lz4_codec, lz4_codec.dumps_many, lz4_codec.loads_many)}
METHOD = {"rans": ("rans", {}), "rans delta": ("rans", dict(rans_delta=True)), "lz4": ("lz4", {})}     # BatchCompressor's arguments


def resident(arrs):
    """-> {name: callable} of the resident encode and decode of arrs for every back-end (checked once against the arrays)."""
    paths, keep = {}, []
    tensors = [torch.from_numpy(a.copy()).to(dev) for a in arrs]
    for name, (codec, comp, decomp) in CODECS.items():
        streams = comp(arrs)
        assert decomp(streams) == [a.tobytes() for a in arrs], name
        up, offs = entropy.upload([entropy.as_bytes(s) for s in streams], dev)
        cap = np.array([a.nbytes for a in arrs], np.int64)
        doff, dend = entropy.aligned_slots(cap)
        meta = torch.from_numpy(np.stack([up.data_ptr() + offs, [len(s) for s in streams], doff, cap]).astype(np.int64)).to(dev)
        dst = torch.empty(dend, dtype=torch.uint8, device=dev)
        keep.append((up, meta, dst))
        paths[name + " encode"] = lambda codec=codec: codec.encode_tensors(tensors)
        paths[name + " decode"] = lambda codec=codec, meta=meta, dst=dst: codec.decode_descriptors(meta[0], meta[1], dst, meta[2], meta[3])
    return paths, keep, tensors


print("\n## 1. %d streams, resident in HBM" % len(arrays))
paths, keep, _ = resident(arrays)
t = measure(paths)
for k in paths:
    print("| %s | %s | %.1f GB/s of array bytes |" % (k, ms(t[k]), raw * B / np.median(t[k]) / 1e9), flush=True)
del paths, keep
torch.cuda.empty_cache()

print("\n## 2. %d streams, host to host" % len(arrays))
paths, streams = {}, {}
for name, (codec, comp, decomp) in CODECS.items():
    streams[name] = comp(arrays)
    paths[name + " compress_many"] = lambda comp=comp: comp(arrays)
    paths[name + " decompress_many"] = lambda decomp=decomp, s=streams[name]: decomp(s)
t = measure(paths)
for k in paths:
    print("| %s | %s |" % (k, ms(t[k])), flush=True)

print("\n## 3. batch pipelines, %d frames" % B)
frames, ids = [xyz] * B, list(range(B))
paths, blobs, keep = {}, {}, []
for name in CODECS:
    bc = pipeline.BatchCompressor(T, cluster_num=M, accuracy=ACC, basic_compressor=METHOD[name][0], seed=1, **METHOD[name][1])
    bd = pipeline.BatchDecompressor(T, M, 2 * ACC, basic_compressor=METHOD[name][0])
    blobs[name] = bc.compress(frames, frame_ids=ids)
    gx, goffs, _, npts = bc._upload(frames)
    up = bd.upload(blobs[name])
    keep.append((bc, bd, gx, goffs, up))

    def resident_compress(bc=bc, gx=gx, goffs=goffs, npts=npts):
        ctx = bc._payload(B, npts, gx, bc.compress_device(gx, goffs, None, ids))
        torch.cuda.synchronize()
        ctx["buf"].in_flight = False
    paths[name + " BatchCompressor.compress"] = lambda bc=bc: bc.compress(frames, frame_ids=ids)
    paths[name + " BatchCompressor resident"] = resident_compress
    paths[name + " BatchDecompressor.decompress"] = lambda bd=bd, b=blobs[name]: bd.decompress(b)
    paths[name + " BatchDecompressor resident"] = lambda bd=bd, b=blobs[name], up=up: bd.decompress_device(b, uploaded=up)
t = measure(paths)
for k in paths:
    print("| %s | %s |" % (k, fps(t[k])), flush=True)
del paths, keep
torch.cuda.empty_cache()

print("\n## 4. one frame's four streams alone, resident")
paths, keep, _ = resident(frame)
host = {"bz2": (lambda a: bz2.compress(a), bz2.decompress), "zlib": (lambda a: zlib.compress(a, 6), zlib.decompress)}
for name, (comp, decomp) in host.items():
    packed = [comp(a.tobytes()) for a in frame]
    paths[name + " (host) encode"] = lambda comp=comp: [comp(a.tobytes()) for a in frame]
    paths[name + " (host) decode"] = lambda decomp=decomp, packed=packed: [decomp(s) for s in packed]
t = measure(paths)
for k in paths:
    print("| %s | %s |" % (k, ms(t[k])), flush=True)

print("\n## 5. container bytes of the example sweep (%d bytes of arrays)" % raw)
sizes = {}
for name, flags in (("lz4", {}), ("deflate", {}), ("bzip2", {})):
    bc = BasicCompressor(method_name=name, **flags)
    sizes[name] = sum(4 + len(bc.compress(a)) for a in frame)
for clog in (14, 15, 16):
    parts = rans_codec.compress_many(frame, chunk_log2=clog)
    sizes["rans, chunk_log2 %d" % clog] = sum(4 + len(s) for s in parts)
    delta = rans_codec.compress_many_delta(frame, chunk_log2=clog)
    sizes["rans delta, chunk_log2 %d" % clog] = sum(4 + len(s) for s in delta)
    if clog == 15:
        for what, ps in (("rans", parts), ("rans delta", delta)):
            print("%s streams at chunk_log2 15:" % what, ", ".join("%s %d (%s %s)" % (k, len(s), s[:2].decode(), "coded" if s[2] else "stored")
                                                                     for k, s in zip(DTYPES, ps)))
        assert sizes["rans, chunk_log2 15"] == len(blobs["rans"][0]) and sizes["rans delta, chunk_log2 15"] == len(blobs["rans delta"][0])
for k, v in sizes.items():
    print("| %s | %d | %.3f of bzip2 |" % (k, v, v / sizes["bzip2"]), flush=True)
