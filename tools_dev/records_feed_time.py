"""GPU: what the NCLT record format (records.py, librpcc_records.so) does to the feed.  N synthetic HDL-32E sweeps
(a few distinct ones, quantised to records and repeated under N file names) are written as record files (8 bytes per point) and as the
float files the reference's preprocessing makes of them (16 bytes per point), and go through loader.StreamingCompressor host to host
(entropy=False: the payload arrives in the pinned output buffers; no entropy coding, no file output) with ingest "nclt", "rows" and
"xyz" taking turns in one process -- "rows" and "xyz" are the baseline, "xyz" loading every file through dataset.load_data on the pool as
tools/compress_datalist.py does.  A turn reads the N files PASSES times over (from the page cache: the files were just written), so that
it lasts about a second; each figure is the median of RUNS turns after a warm-up turn of every ingest, and the spread (min .. max) is
printed beside it.  Also: the bytes that cross the link per frame, and the unpack launch alone (device events around REPS back-to-back
calls on one batch's records) in microseconds and bytes per second, beside the HBM rate a float4 copy reaches on this device
(6.29 TB/s measured, MI355X microarchitecture notes; a batch's records and rows together are smaller than the 256 MiB last-level cache, so
back-to-back launches on one buffer can exceed it).
Usage: python tools_dev/records_feed_time.py [--frames 1024] [--passes 20] [--batch 128] [--dir DIR] [--json FILE]"""
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
import records_ref as R  # noqa: E402  (pack_ref: records of synthetic sweeps)
from rpcc_amd import records  # noqa: E402
from rpcc_amd.dataset import build_dataset  # noqa: E402
from rpcc_amd.loader import StreamingCompressor  # noqa: E402
from rpcc_amd.pipeline import BatchCompressor  # noqa: E402

RUNS, REPS, DISTINCT = 3, 200, 8
HBM_COPY_BYTES_PER_S = 6.29e12
THREADS = int(os.environ.get("OMP_NUM_THREADS", "16"))   # the CPUs this job may use, not the machine's


def write_files(d, n):
    recs = [R.synthetic_records(9500 + i) for i in range(DISTINCT)]
    rec_paths, row_paths = [], []
    for k in range(n):
        r = recs[k % DISTINCT]
        rec_paths.append(os.path.join(d, "sync_%06d.bin" % k))
        r.tofile(rec_paths[-1])
        rows = records.unpack_host(r)
        rows[:, 3] = 0          # preprocess_original_utf8_to_bin_file writes zeros there
        row_paths.append(os.path.join(d, "pre_%06d.bin" % k))
        rows.tofile(row_paths[-1])
    return recs, rec_paths, row_paths


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--passes", type=int, default=20, help="times a turn goes through the files")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--dir", default=None, help="where the files are written (default: a temporary directory)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    dev = torch.device("cuda:0")
    ds = build_dataset(lidar_type="Velodyne32E")
    T = ds.PCTransformer
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        recs, rec_paths, row_paths = write_files(d, a.frames)
        points = float(np.mean([recs[k % DISTINCT].shape[0] for k in range(a.frames)]))
        out = dict(frames=a.frames, passes=a.passes, batch=a.batch, points_per_frame=round(points, 1), runs=RUNS, threads=THREADS, geometry="Velodyne32E 32x2250",
                   ingest={})
        pool = ThreadPoolExecutor(THREADS)
        paths = dict(nclt=rec_paths, rows=row_paths, xyz=row_paths)
        per_point = dict(nclt=8, rows=16, xyz=12)
        scs = {k: StreamingCompressor(BatchCompressor(T, cluster_num=100, accuracy=0.02, seed=1), batch=a.batch, depth=4, workers=THREADS,
                                      pool=pool, ingest=k) for k in paths}
        ids = list(range(a.frames))

        def batches(kind, passes):
            for _ in range(passes):
                for s in range(0, a.frames, a.batch):
                    names = paths[kind][s: s + a.batch]
                    yield (list(pool.map(ds.load_data, names)) if kind == "xyz" else names), ids[s: s + a.batch]

        def turn(kind, passes=a.passes):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = scs[kind].run(batches(kind, passes), sink=None, entropy=False)      # returns after the last batch's payload is on the host
            dt = time.perf_counter() - t0
            assert n == a.frames * passes
            return n / dt

        for kind in paths:          # warm-up: code objects, slot growth, page cache
            turn(kind, 2)
        rates = {k: [] for k in paths}
        for _ in range(RUNS):       # the three take turns
            for kind in paths:
                rates[kind].append(turn(kind))
        for kind, v in rates.items():
            out["ingest"][kind] = dict(frames_per_s=round(statistics.median(v), 1), min=round(min(v), 1), max=round(max(v), 1),
                                       seconds_per_turn=round(a.frames * a.passes / statistics.median(v), 2),
                                       link_bytes_per_frame=int(per_point[kind] * points), grown=scs[kind].grown)
        out["nclt_over_rows"] = round(out["ingest"]["nclt"]["frames_per_s"] / out["ingest"]["rows"]["frames_per_s"], 3)
        out["nclt_over_xyz"] = round(out["ingest"]["nclt"]["frames_per_s"] / out["ingest"]["xyz"]["frames_per_s"], 3)

        # the unpack launch alone, on one batch's records
        batch = torch.from_numpy(np.concatenate([recs[k % DISTINCT] for k in range(a.batch)])).to(dev)
        rows = torch.empty((batch.shape[0], 4), dtype=torch.float32, device=dev)
        records.unpack(batch, out=rows)
        torch.cuda.synchronize()
        assert np.array_equal(rows[: recs[0].shape[0]].cpu().numpy().view(np.uint32), records.unpack_host(recs[0]).view(np.uint32))
        us = []
        for _ in range(RUNS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(REPS):
                records.unpack(batch, out=rows)
            e1.record()
            torch.cuda.synchronize()
            us.append(1e3 * e0.elapsed_time(e1) / REPS)
        t = statistics.median(us)
        nbytes = 24 * batch.shape[0]        # 8 read, 16 written per point
        out["unpack"] = dict(points=int(batch.shape[0]), us=round(t, 2), min_us=round(min(us), 2), max_us=round(max(us), 2), bytes=nbytes,
                             bytes_per_s=round(nbytes / (t * 1e-6), -9), share_of_hbm_copy_rate=round(nbytes / (t * 1e-6) / HBM_COPY_BYTES_PER_S, 3),
                             hbm_copy_bytes_per_s=HBM_COPY_BYTES_PER_S)
        pool.shutdown()
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
