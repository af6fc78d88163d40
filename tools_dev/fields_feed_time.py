"""GPU: what reading .pcd files on the device (pointfile.py, librpcc_fields.so) does to the feed.  N synthetic HDL-32E
sweeps of about 52.7 k points (a few distinct ones, repeated under N file names) are written as PCL PointXYZI .pcd files (32-byte records),
as the same records `binary_compressed`, and as .bin rows, and go through loader.StreamingCompressor host to host (entropy=False: the
payload arrives in the pinned output buffers; no entropy coding, no file output), the four ways taking turns in one process:
  pcd32_fields       the .pcd files through ingest "fields" (read in place, unpacked on the device)
  bin_rows           the same points as .bin through ingest "rows"
  pcd32_xyz          the same .pcd files through dataset.load_data on the pool and ingest "xyz": the reference-style load
  compressed_fields  the binary_compressed files through ingest "fields" (LZF on the workers)
A turn reads the N files PASSES times over (from the page cache: the files were just written); each figure is the median of RUNS turns after a
warm-up turn of every way, with the spread (min .. max) beside it.  Also the unpack launch alone for records of 12, 16, 22 and 32 bytes
(device events around REPS back-to-back calls on one batch) in microseconds and bytes moved per second (step + 16 per point), beside the
record unpack's figure (162 MB in 25 us).
Usage: python tools_dev/fields_feed_time.py [--frames 512] [--passes 10] [--batch 128] [--dir DIR] [--json FILE]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rpcc_amd  # noqa: E402,F401
import fields_ref as FR  # noqa: E402  (record_frame: synthetic records of a given step)
import pointfile_cases as PC  # noqa: E402  (packed / planes / compressed / pcd: the files)
import records_ref as R  # noqa: E402  (synthetic sweeps)
from rpcc_amd import pointfile, records  # noqa: E402
from rpcc_amd.dataset import build_dataset  # noqa: E402
from rpcc_amd.loader import StreamingCompressor  # noqa: E402
from rpcc_amd.pipeline import BatchCompressor  # noqa: E402

RUNS, REPS, DISTINCT = 3, 100, 4
RECORD_UNPACK_BYTES_PER_S = 162e6 / 25e-6
THREADS = int(os.environ.get("OMP_NUM_THREADS", "16"))   # the CPUs this job may use, not the machine's
FIELDS, SIZE, KIND, COUNT = ["x", "y", "z", "_", "intensity", "_"], (4, 4, 4, 1, 4, 1), "FFFUFU", (1, 1, 1, 4, 1, 12)


def cols(rows):
    x, y, z, w = (np.ascontiguousarray(rows[:, c]) for c in range(4))
    return [("x", "<f4", x), ("y", "<f4", y), ("z", "<f4", z), ("_", ("u1", 4), None), ("intensity", "<f4", w), ("_", ("u1", 12), None)]


def write_files(d, n):
    sweeps = [records.unpack_host(R.synthetic_records(9500 + i)) for i in range(DISTINCT)]
    blobs = []
    for rows in sweeps:
        body, step = PC.packed(cols(rows))
        assert step == 32
        blobs.append((PC.pcd(FIELDS, SIZE, KIND, body, rows.shape[0], count=COUNT),
                      PC.pcd(FIELDS, SIZE, KIND, PC.compressed(PC.planes(cols(rows))), rows.shape[0], count=COUNT, data="binary_compressed"), rows.tobytes()))
    paths = dict(pcd=[], comp=[], bin=[])
    for k in range(n):
        for kind, blob, ext in zip(("pcd", "comp", "bin"), blobs[k % DISTINCT], ("pcd", "pcd", "bin")):
            paths[kind].append(os.path.join(d, "%s_%06d.%s" % (kind, k, ext)))
            with open(paths[kind][-1], "wb") as f:
                f.write(blob)
    assert np.array_equal(pointfile.read_rows(paths["comp"][0]).view(np.uint32), sweeps[0].view(np.uint32))
    assert np.array_equal(pointfile.read_rows(paths["pcd"][0]).view(np.uint32), sweeps[0].view(np.uint32))
    return sweeps, paths, [len(b[1]) for b in blobs]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--passes", type=int, default=10, help="times a turn goes through the files")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--dir", default=None, help="where the files are written (default: a temporary directory)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    dev = torch.device("cuda:0")
    ds = build_dataset(lidar_type="Velodyne32E")
    T = ds.PCTransformer
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        sweeps, paths, comp_bytes = write_files(d, a.frames)
        points = float(np.mean([sweeps[k % DISTINCT].shape[0] for k in range(a.frames)]))
        out = dict(frames=a.frames, passes=a.passes, batch=a.batch, points_per_frame=round(points, 1), runs=RUNS, threads=THREADS, geometry="Velodyne32E 32x2250",
                   compressed_file_bytes=int(np.mean(comp_bytes)), ways={})
        pool = ThreadPoolExecutor(THREADS)
        ways = dict(pcd32_fields=("fields", "pcd"), bin_rows=("rows", "bin"), pcd32_xyz=("xyz", "pcd"), compressed_fields=("fields", "comp"))
        link = dict(pcd32_fields=32 * points, bin_rows=16 * points, pcd32_xyz=12 * points, compressed_fields=32 * points)
        scs = {k: StreamingCompressor(BatchCompressor(T, cluster_num=100, accuracy=0.02, seed=1), batch=a.batch, depth=4, workers=THREADS,
                                      pool=pool, ingest=v[0]) for k, v in ways.items()}
        ids = list(range(a.frames))

        def batches(way, passes):
            ingest, files = ways[way]
            for _ in range(passes):
                for s in range(0, a.frames, a.batch):
                    names = paths[files][s: s + a.batch]
                    yield (list(pool.map(ds.load_data, names)) if ingest == "xyz" else names), ids[s: s + a.batch]

        def turn(way, passes=a.passes):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = scs[way].run(batches(way, passes), sink=None, entropy=False)      # returns after the last batch's payload is on the host
            dt = time.perf_counter() - t0
            assert n == a.frames * passes
            return n / dt

        for way in ways:          # warm-up: code objects, slot growth, page cache
            turn(way, 2)
        rates = {k: [] for k in ways}
        for _ in range(RUNS):       # the four take turns
            for way in ways:
                rates[way].append(turn(way))
        for way, v in rates.items():
            out["ways"][way] = dict(frames_per_s=round(statistics.median(v), 1), min=round(min(v), 1), max=round(max(v), 1),
                                    seconds_per_turn=round(a.frames * a.passes / statistics.median(v), 2), link_bytes_per_frame=int(link[way]),
                                    grown=scs[way].grown)
        for k in ("bin_rows", "pcd32_xyz"):
            out["pcd32_fields_over_" + k] = round(out["ways"]["pcd32_fields"]["frames_per_s"] / out["ways"][k]["frames_per_s"], 3)
        pool.shutdown()

    # the unpack launch alone, on one batch of records of each step
    rng = np.random.default_rng(1)
    n = int(points)
    out["unpack"] = {}
    for step, types in ((12, (FR.F32, FR.F32, FR.F32, FR.NONE)), (16, (FR.F32,) * 4), (22, (FR.F32,) * 4), (32, (FR.F32,) * 4)):
        data, d0, want = FR.record_frame(rng, n, step, types=types)
        head = 11 if step == 22 else 0                      # behind a header of odd length
        slot = (head + len(data) + 15) & ~15
        chunk = np.zeros(slot * a.batch, np.uint8)
        desc = np.zeros((a.batch, pointfile.DESC_WORDS), np.int64)
        for b in range(a.batch):
            chunk[b * slot + head: b * slot + head + len(data)] = np.frombuffer(data, np.uint8)
            desc[b] = d0
            desc[b, 0] = b * slot + head
        chunk_dev, desc_dev = torch.from_numpy(chunk).to(dev), torch.from_numpy(desc).to(dev)
        offs_dev = torch.arange(a.batch + 1, dtype=torch.int64, device=dev) * n
        total = n * a.batch
        rows = torch.empty((total, 4), dtype=torch.float32, device=dev)
        status = torch.empty((a.batch,), dtype=torch.int32, device=dev)
        pointfile.unpack_into(chunk_dev, desc_dev, offs_dev, total, rows, status)
        torch.cuda.synchronize()
        assert not status.any().item() and np.array_equal(rows[-n:].cpu().numpy().view(np.uint32), want.view(np.uint32))
        us = []
        for _ in range(RUNS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(REPS):
                pointfile.unpack_into(chunk_dev, desc_dev, offs_dev, total, rows, status)
            e1.record()
            torch.cuda.synchronize()
            us.append(1e3 * e0.elapsed_time(e1) / REPS)
        t = statistics.median(us)
        nbytes = (step + 16) * total
        out["unpack"]["step%d" % step] = dict(points=total, us=round(t, 2), min_us=round(min(us), 2), max_us=round(max(us), 2), bytes=nbytes,
                                              bytes_per_s=round(nbytes / (t * 1e-6), -9),
                                              share_of_record_unpack_rate=round(nbytes / (t * 1e-6) / RECORD_UNPACK_BYTES_PER_S, 3))
        del chunk_dev, rows
    out["record_unpack_bytes_per_s"] = RECORD_UNPACK_BYTES_PER_S
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
