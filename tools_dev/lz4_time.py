"""GPU: time of the LZ4 back-end (librpcc_lz4.so) on a 256-frame batch of 64 x 2048-class arrays: encode + container compaction
and decode (device events, after a warm-up, inputs already in HBM), BatchCompressor end to end with 'lz4' against 'bzip2' (three
batches in flight, wall clock), and -- labelled as a CPU number -- the system liblz4's LZ4_compress_default on 16 threads over the
same arrays where it loads.  The arrays are the example sweep's (tests/golden/example_64E.npz): contour bits, index sequence,
models and residuals, one copy per frame, uniform framework.
Kernel times: run it under `rocprofv3 --kernel-trace --stats -d <dir> -- python tools_dev/lz4_time.py --reps 3`.
Usage: python tools_dev/lz4_time.py [--frames 256] [--reps N] [--json FILE]"""
import argparse
import ctypes
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
from rpcc_amd import _lz4_lib as L  # noqa: E402
from rpcc_amd import lz4_codec  # noqa: E402
from rpcc_amd._lib import ptr, stream  # noqa: E402

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

    state = {}

    def enc():
        slots, dst_off, dst_len, _ = lz4_codec.encode_descriptors(desc[0], desc[1], caps)
        out, frame = lz4_codec.pack_containers(slots, dst_off, dst_len, B, k, slots.numel() + 4 * len(arrays))
        state.update(slots=slots, dst_off=dst_off, dst_len=dst_len, out=out, frame=frame)

    ms = timed(enc, args.reps)
    res["encode_pack_ms"] = ms
    res["encode_pack_GBps"] = nbytes / ms / 1e6
    res["encode_pack_frames_per_s"] = B / ms * 1e3
    # the containers equal dumps_many's streams (a spot check on frame 0 of the batch)
    fr = state["frame"].cpu().numpy()
    blob = state["out"][int(fr[0, 0]): int(fr[0, 0] + fr[1, 0])].cpu().numpy().tobytes()
    want = b"".join(len(b).to_bytes(4, "little") + b for b in lz4_codec.dumps_many(per))
    assert blob == want, "container mismatch"
    res["compressed_bytes_per_frame"] = int(fr[1, 0])

    # decode the batch's streams from the encoder's slots into one buffer
    slots, dst_off, dst_len = state["slots"], state["dst_off"], state["dst_len"]
    src_addr = slots.data_ptr() + dst_off
    out = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    doff = torch.from_numpy(offs.astype(np.int64)).to(dev)
    dcap = desc[1]
    dlen = torch.empty(len(arrays), dtype=torch.int64, device=dev)
    st = torch.empty(len(arrays), dtype=torch.int32, device=dev)

    def dec():
        L.check(L.lib().rpcc_lz4_decode(ptr(src_addr), ptr(dst_len), len(arrays), ptr(out), ptr(doff), ptr(dcap), ptr(dlen), ptr(st), stream()))

    ms = timed(dec, args.reps)
    assert int((st != 0).sum()) == 0 and torch.equal(out, data), "decode mismatch"
    res["decode_ms"] = ms
    res["decode_GBps"] = nbytes / ms / 1e6
    res["decode_frames_per_s"] = B / ms * 1e3

    # BatchCompressor end to end, three batches in flight, 'lz4' against 'bzip2' (bzip2 on the host pool, as the datalist tool runs it)
    from oracle import oracle as orc
    from rpcc_amd import dataset, synth
    from rpcc_amd.pipeline import BatchCompressor
    gd = orc.GEOMS["Velodyne64E_2048"]
    T = dataset.build_dataset(lidar_type="Velodyne64E_2048").PCTransformer
    nb = min(B, 64)
    frames = [synth.make_frame(5000 + i, gd["H"], gd["W"], vmax_deg=gd["vmax_deg"], vmin_deg=gd["vmin_deg"]).numpy() for i in range(nb)]
    with ThreadPoolExecutor(THREADS) as pool:
        for m in ("lz4", "bzip2"):
            bc = BatchCompressor(T, basic_compressor=m, seed=1)
            bc.collect(bc.submit(frames), pool=pool)   # warm-up
            torch.cuda.synchronize()
            t = time.perf_counter()
            ctxs = [bc.submit(frames) for _ in range(3)]
            got = [bc.collect(c, pool=pool) for c in ctxs]
            dt = time.perf_counter() - t
            res["batch_%s_frames_per_s" % m] = 3 * nb / dt
            res["batch_%s_bytes_per_frame" % m] = float(np.mean([len(b) for b in got[0]]))

    try:
        lz = ctypes.CDLL("liblz4.so.1")
    except OSError:
        lz = None
    if lz is not None:
        dst = [ctypes.create_string_buffer(lz.LZ4_compressBound(len(a))) for a in arrays]

        def one(i):
            return lz.LZ4_compress_default(arrays[i], dst[i], len(arrays[i]), len(dst[i]))

        with ThreadPoolExecutor(THREADS) as pool:
            list(pool.map(one, range(len(arrays))))
            t = time.perf_counter()
            list(pool.map(one, range(len(arrays))))
            dt = time.perf_counter() - t
        res["cpu_liblz4_threads"] = THREADS
        res["cpu_liblz4_GBps"] = nbytes / dt / 1e9
        res["cpu_liblz4_frames_per_s"] = B / dt
    print(json.dumps(res))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
