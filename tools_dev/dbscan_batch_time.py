"""GPU: DBSCAN through the batch front-end (pipeline.BatchCompressor(segment_method="DBSCAN")) against the per-frame
stages of tools/compress.py, on synthetic 64 x 2048 sweeps, eps 1.5: 256 frames in batches of 32 (32 different sweeps, taken eight times
under different frame identities).  Three numbers, each the median of 3 runs after a warm-up of every shape:
  * host to host: frames in host memory -> .rpcc byte strings (bzip2), the next batch submitted before the last is collected, the entropy
    coder on a pool of the job's CPUs;
  * the device part of a batch alone (device events), split into projection + ground fit, dbscan_segment, ops.compress_batch_labels
    (label intake and everything behind it) and contour codec + payload packing.  The label intake's own time is a kernel time: run this
    tool under `rocprofv3 --kernel-trace --stats -d <dir> -- python tools_dev/dbscan_batch_time.py --device-only` and read labels_in_kernel;
  * the same frames through PointCloudSegment.segment / cluster_modeling / intra_predict / quantize_residual / compress_point_cloud /
    pack_bitstream one by one: the only way before the batch path existed, and the baseline.
Usage: python tools_dev/dbscan_batch_time.py [--frames 256] [--batch 32] [--per-frame 32] [--device-only] [--json FILE]"""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rpcc_amd  # noqa: E402,F401
from rpcc_amd import compress_utils as cu, ops, synth  # noqa: E402
from rpcc_amd.dbscan import dbscan_segment  # noqa: E402
from rpcc_amd.pipeline import BatchCompressor  # noqa: E402
from rpcc_amd.segment_utils import PointCloudSegment  # noqa: E402
from rpcc_amd.transformer import PCTransformer  # noqa: E402

H, W, VMAX, VMIN, EPS, ACC, SEED = 64, 2048, 2.0, -24.9, 1.5, 0.04, 1
RUNS = 3
THREADS = int(os.environ.get("OMP_NUM_THREADS", "16"))   # the CPUs this job may use, not the machine's


def device_ms(fn):
    """fn() on the current stream between two events -> milliseconds (the stream is drained before and after)."""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def device_split(bc, batches):
    """Per batch: ms of [projection + ground fit, dbscan_segment, compress_batch_labels, contour codec + payload packing]."""
    T, tm = bc.T, bc.T.tm_dev
    rows = []
    for frames, ids in batches:
        xyz, offs, _, npts = bc._upload(frames)
        buf = bc._buffers(len(frames))
        ground = torch.zeros((len(frames), 4), dtype=torch.float64, device=bc.device)

        def front():
            ops.project(xyz, offs, T.geom, ri=buf.ri)
            g, _ = ops.ground_ransac(buf.ri, tm, seed=bc.seed, frame_ids=ids)
            ground.copy_(g)
        t_front, _ = device_ms(front)
        t_seg, (labels, top) = device_ms(lambda: dbscan_segment(buf.ri, tm, ground, bc.eps, min_points=10, check=False))
        t_lab, _ = device_ms(lambda: ops.compress_batch_labels(buf.ri, tm, ground, labels, top, buf, bc.acc, plane_seed=bc.seed, frame_ids=ids))

        def back():
            bits, seq, nseq = ops.contour_encode(buf.seg, bc.M, ws=buf.codec_ws)
            ops.pack_payload(buf.q16, buf.nnz, capacity=npts)
            ops.pack_payload(seq.view(torch.int16), nseq)
        t_back, _ = device_ms(back)
        assert not buf.status.any()
        rows.append((t_front, t_seg, t_lab, t_back))
    return np.array(rows)


def host_to_host(bc, batches, pool):
    t0 = time.perf_counter()
    n, pending = 0, None
    for frames, ids in batches:
        ctx = bc.submit(frames, frame_ids=ids)
        if pending is not None:
            n += len(bc.collect(pending, pool=pool))
        pending = ctx
    n += len(bc.collect(pending, pool=pool))
    return n / (time.perf_counter() - t0)


def per_frame(T, frames, ids):
    """tools/compress.py's stages, frame by frame -> frames/s (host to host, bzip2)."""
    bz = cu.BasicCompressor(method_name="bzip2")
    cfg = {"segment_method": "DBSCAN", "ground_vertical_threshold": 0.1, "cluster_num": 100, "DBSCAN_eps": EPS}
    t0 = time.perf_counter()
    for f, i in zip(frames, ids):
        ri = np.expand_dims(T.point_cloud_to_range_image(f), -1)
        pc = T.range_image_to_point_cloud(ri)
        ps = PointCloudSegment(T.transform_map, seed=SEED, frame_id=i)
        seg_idx, gm = ps.segment(pc, ri, cfg)
        model_param = np.concatenate((gm.reshape(1, 4), ps.cluster_modeling(pc, ri, seg_idx, {"model_method": "point", "angle_threshold": 75})), 0)
        residual = ri - ps.intra_predict(seg_idx, model_param)
        rq, sal, _ = cu.QuantizationModule(ACC).quantize_residual(residual, seg_idx, pc, ri)
        _, compressed = cu.compress_point_cloud(bz, model_param, seg_idx, sal, rq, full=False)
        cu.pack_bitstream(compressed, uniform=True)
    return len(frames) / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--per-frame", dest="per_frame", type=int, default=32, help="frames of the per-frame baseline per run")
    ap.add_argument("--device-only", dest="device_only", action="store_true", help="the device part only, one run (for a profiler)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    B = a.batch
    T = PCTransformer(dict(HORIZONTAL_FOV=360, VERTICAL_ANGLE_MAX=VMAX, VERTICAL_ANGLE_MIN=VMIN, RANGE_IMAGE_HEIGHT=H, RANGE_IMAGE_WIDTH=W))
    base = [synth.make_frame(i, H, W, vmax_deg=VMAX, vmin_deg=VMIN, device="cuda:0").cpu().numpy() for i in range(B)]
    batches = [(base, list(range(k * B, k * B + B))) for k in range(a.frames // B)]
    bc = BatchCompressor(T, accuracy=ACC / 2, seed=SEED, segment_method="DBSCAN", DBSCAN_eps=EPS)
    out = dict(frames=a.frames, batch=B, eps=EPS, runs=RUNS, threads=THREADS)
    device_split(bc, batches[:1])                                            # warm-up of every launch
    dev = [device_split(bc, batches) for _ in range(1 if a.device_only else RUNS)]
    per_batch = np.median(np.stack([d.sum(0) / len(batches) for d in dev]), 0)   # ms per batch of each part, median over the runs
    out["device_ms_per_frame"] = dict(zip(("project_ground", "dbscan", "labels_entry", "contour_pack"), (per_batch / B).round(4).tolist()))
    out["device_frames_per_s"] = round(1e3 * B / float(per_batch.sum()), 1)
    if not a.device_only:
        with ThreadPoolExecutor(THREADS) as pool:
            host_to_host(bc, batches[:2], pool)
            out["batch_host_to_host_frames_per_s"] = round(statistics.median(host_to_host(bc, batches, pool) for _ in range(RUNS)), 1)
        n = min(a.per_frame, B)
        per_frame(T, base[:2], [0, 1])
        out["per_frame_host_to_host_frames_per_s"] = round(statistics.median(per_frame(T, base[:n], list(range(n))) for _ in range(RUNS)), 2)
        out["per_frame_frames_timed"] = n
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
