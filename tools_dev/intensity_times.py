"""GPU: what the intensity channel costs, on copies of the example sweep (tests/golden/example_64E.npz with the
fourth column of tests/golden/intensity_example_64E.npz: 122 320 rows, 64 x 2000), the rows resident in HBM:
  * ops.intensity_encode against rpcc_project_strided on the same rows (both read every point and compute every pixel), --frames copies;
  * BatchCompressor.compress and BatchDecompressor.decompress, host to host, with and without intensity, for 'rans' and 'bzip2',
    --pipeline-frames copies (frames/s);
  * the size of the example container at scale 100 and 255, and without intensity, for every back-end.
Each time is the median of RUNS runs after a warm-up; the compared items take turns inside one process.
Usage: python tools_dev/intensity_times.py [--frames 256] [--pipeline-frames 256] [--json FILE]"""
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
from rpcc_amd import compress_utils as cu  # noqa: E402
from rpcc_amd import ops, pipeline  # noqa: E402
from rpcc_amd.dataset import build_dataset  # noqa: E402

RUNS = 3
GOLDEN = os.path.join(ROOT, "tests", "golden")


def device_ms(fn, reps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def host_s(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def turns(fns, measure):
    """Median over RUNS rounds in which the items take turns (after one warm-up round)."""
    for f in fns.values():
        f()
    got = {k: [] for k in fns}
    for _ in range(RUNS):
        for k, f in fns.items():
            got[k].append(measure(f))
    return {k: dict(median=statistics.median(v), min=min(v), max=max(v)) for k, v in got.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--pipeline-frames", dest="pipeline_frames", type=int, default=256)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    T = build_dataset(lidar_type="Velodyne64E").PCTransformer
    xyz = np.load(os.path.join(GOLDEN, "example_64E.npz"))["xyz"]
    k = np.load(os.path.join(GOLDEN, "intensity_example_64E.npz"))["k"]
    one = np.ascontiguousarray(np.concatenate([xyz, (k.astype(np.float32) / np.float32(100))[:, None]], 1), dtype=np.float32)
    n, P = one.shape[0], T.H * T.W
    out = dict(points_per_frame=n, runs=RUNS)

    # 1. the kernels alone
    B = a.frames
    rows = torch.from_numpy(one).to(dev).repeat(B, 1).contiguous()
    offs = torch.arange(B + 1, dtype=torch.int64, device=dev) * n
    ri = torch.empty((B, T.H, T.W), dtype=torch.float32, device=dev)
    s_proj = torch.empty(ops._lib.lib().rpcc_project_scratch_bytes(B * n, B, P), dtype=torch.uint8, device=dev)
    s_int = torch.empty(ops._lib.lib().rpcc_intensity_scratch_bytes(B, P), dtype=torch.uint8, device=dev)
    pay, nb, orph = torch.empty((B, 8 + P), dtype=torch.uint8, device=dev), torch.empty((B,), dtype=torch.int32, device=dev), torch.empty((B,), dtype=torch.int32, device=dev)
    ops.project(rows, offs, T.geom, ri=ri, scratch=s_proj)
    seg = torch.where(ri != 0, 2, 1).to(torch.uint8)
    w = torch.empty_like(ri)
    st = torch.empty((B,), dtype=torch.int32, device=dev)
    ker = turns(dict(project_strided=lambda: ops.project(rows, offs, T.geom, ri=ri, scratch=s_proj),
                     intensity_encode=lambda: ops.intensity_encode(rows, offs, T.geom, ri, 100.0, payload=pay, nbytes=nb, orphans=orph, scratch=s_int),
                     intensity_decode=lambda: ops.intensity_decode(pay, nb, seg, out=w, status=st)), lambda f: device_ms(f, 10))
    assert not orph.any() and not st.any()
    out["kernels_ms"] = dict(frames=B, **ker, encode_over_project=ker["intensity_encode"]["median"] / ker["project_strided"]["median"])
    del rows, ri, s_proj, s_int, pay, seg, w
    torch.cuda.empty_cache()

    # 2. the pipelines, host to host
    Bp = a.pipeline_frames
    frames4, frames3 = [one] * Bp, [one[:, :3]] * Bp
    out["pipeline_frames_per_s"] = {}
    blobs = {}
    for method in ("rans", "bzip2"):
        bc_w = pipeline.BatchCompressor(T, basic_compressor=method, intensity_scale=100.0)
        bc_0 = pipeline.BatchCompressor(T, basic_compressor=method)
        keep = {}
        enc = turns(dict(plain=lambda: keep.__setitem__("plain", bc_0.compress(frames3)), intensity=lambda: keep.__setitem__("intensity", bc_w.compress(frames4))), host_s)
        bd_w = pipeline.BatchDecompressor(T, 100, 0.04, basic_compressor=method, intensity=True)
        bd_0 = pipeline.BatchDecompressor(T, 100, 0.04, basic_compressor=method)
        dec = turns(dict(plain=lambda: bd_0.decompress(keep["plain"]), intensity=lambda: bd_w.decompress(keep["intensity"])), host_s)
        out["pipeline_frames_per_s"][method] = dict(frames=Bp, compress={k_: Bp / v["median"] for k_, v in enc.items()},
                                                    decompress={k_: Bp / v["median"] for k_, v in dec.items()},
                                                    compress_s=enc, decompress_s=dec)
        blobs[method] = keep

    # 3. sizes of the example container
    sizes = {}
    for method, kw in (("lz4", {}), ("bzip2", {}), ("gzip", {}), ("deflate", {}), ("rans", {}), ("rans", dict(rans_delta=True))):
        name = method + ("_delta" if kw else "")
        sizes[name] = {}
        for label, scale in (("none", None), ("scale_100", 100.0), ("scale_255", 255.0)):
            bc = pipeline.BatchCompressor(T, basic_compressor=method, intensity_scale=scale, **kw)
            blob = bc.compress([one if scale else one[:, :3]])[0]
            span = cu.intensity_trailer_span(blob) if scale else None
            sizes[name][label] = dict(container=len(blob), trailer=(span[1] - span[0] + 4) if span else 0)
    out["example_container_bytes"] = sizes
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
