"""GPU: what the hidden_points channel costs and what it buys, on the example sweep (tests/golden/example_64E.npz:
122 320 rows, 64 x 2000):
  * ops.hidden_encode / hidden_decode at bits 0 and 2 beside ops.subpixel_encode / subpixel_decode on the same rows, --frames copies
    resident in HBM (the owner pass is shared work; the count pass sends every row through the exact projection sequence);
  * at accuracy 0.02 with bzip2, for (subpixel off | 2) x (hidden_points off | on): the container's bytes, the carried and uncarried
    counts, and Chamfer distance, F-score, D1 / D2 PSNR of the decoded points (evaluate_metrics) against the ORIGINAL example points.
    The condition checked: Chamfer with the trailer is strictly smaller than without it, at both widths, and nothing is uncarried.
Each time is the median of RUNS runs after a warm-up (min - max beside it); the compared items take turns inside one process.
Usage: python tools_dev/hidden_times.py [--frames 256] [--json FILE]; exit status 1 when the condition does not hold."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rpcc_amd  # noqa: E402,F401
from intensity_times import GOLDEN, RUNS, device_ms, turns  # noqa: E402
from rpcc_amd import compress_utils as cu  # noqa: E402
from rpcc_amd import ops, pipeline  # noqa: E402
from rpcc_amd.dataset import build_dataset  # noqa: E402
from rpcc_amd.evaluate_metrics import calc_chamfer_distance, calc_point_to_point_plane_psnr  # noqa: E402
from rpcc_amd.tools.decompress import decode_frame  # noqa: E402

ACCURACY, BITS = 0.02, (0, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    T = build_dataset(lidar_type="Velodyne64E").PCTransformer
    xyz = np.load(os.path.join(GOLDEN, "example_64E.npz"))["xyz"]
    one = np.ascontiguousarray(np.concatenate([xyz, np.zeros((xyz.shape[0], 1), np.float32)], 1), dtype=np.float32)
    n, P = one.shape[0], T.H * T.W
    out = dict(points_per_frame=n, runs=RUNS, accuracy=ACCURACY)

    # 1. the kernels alone
    B = a.frames
    L = ops._lib.lib()
    rows = torch.from_numpy(one).to(dev).repeat(B, 1).contiguous()
    offs = torch.arange(B + 1, dtype=torch.int64, device=dev) * n
    ri = ops.project(rows, offs, T.geom)
    u8, i32 = (lambda *s: torch.empty(s, dtype=torch.uint8, device=dev)), (lambda *s: torch.empty(s, dtype=torch.int32, device=dev))
    s_sub, s_hid = u8(L.rpcc_subpixel_scratch_bytes(B, P)), u8(L.rpcc_hidden_scratch_bytes(B, P, B * n))
    spay, snb, sorph = u8(B, 8 + 2 * P), i32(B), i32(B)
    hpay, hnb, horph, hunc = {b: u8(B, ops.hidden_row_bytes(P, n)) for b in BITS}, i32(B), i32(B), i32(B)
    seg = torch.where(ri != 0, 2, 1).to(torch.uint8)
    pts, st, cnt = torch.empty((B, T.H, T.W, 3), dtype=torch.float32, device=dev), i32(B), i32(B)
    tab, tm = T.subpixel_tables(), T.tm_dev
    fns = dict(subpixel_encode_2=lambda: ops.subpixel_encode(rows, offs, T.geom, ri, 2, payload=spay, nbytes=snb, orphans=sorph, scratch=s_sub),
               subpixel_decode_2=lambda: ops.subpixel_decode(spay, snb, seg, ri, tab, out=pts, status=st))
    for bits in BITS:
        fns["hidden_encode_%d" % bits] = lambda bits=bits: ops.hidden_encode(rows, offs, T.geom, ri, 2 * ACCURACY, bits, payload=hpay[bits], nbytes=hnb,
                                                                                 orphans=horph, uncarried=hunc, scratch=s_hid)
    ops.hidden_encode(rows, offs, T.geom, ri, 2 * ACCURACY, 0, payload=hpay[0], nbytes=hnb, orphans=horph, uncarried=hunc, scratch=s_hid)
    m = int(np.frombuffer(hpay[0][0, 12:16].cpu().numpy().tobytes(), "<u4")[0])
    hpts = torch.empty((B, m, 3), dtype=torch.float32, device=dev)
    nb_of = {}
    for bits in BITS:       # the payloads the decoders read, made once (hnb is shared: a copy per width)
        fns["hidden_encode_%d" % bits]()
        nb_of[bits] = hnb.clone()
        fns["hidden_decode_%d" % bits] = lambda bits=bits: ops.hidden_decode(hpay[bits], nb_of[bits], seg, tm, tab, out=hpts, count=cnt, status=st)
    ker = turns(fns, lambda f: device_ms(f, 10))
    assert not horph.any() and not sorph.any() and not st.any() and not hunc.any() and int(cnt[0]) == m
    out["kernels_ms"] = dict(frames=B, hidden_points_per_frame=m, **ker)
    del rows, ri, s_sub, s_hid, spay, hpay, seg, pts, hpts
    torch.cuda.empty_cache()

    # 2. size and quality of the example container, bzip2, against the original points
    host = cu.BasicCompressor(method_name="bzip2")
    quality = {}
    for sub in (None, 2):
        for hid in (False, True):
            bc = pipeline.BatchCompressor(T, accuracy=ACCURACY, basic_compressor="bzip2", subpixel_bits=sub, hidden_points=hid)
            blob = bc.compress([one[:, :3]])[0]
            cd = cu.unpack_bitstream(blob, subpixel=sub is not None, hidden_points=hid)
            pc = decode_frame(cd, host, T, 100, 2 * ACCURACY, None, True, subpixel=sub is not None, hidden_points=hid)[1].reshape(-1, 3)
            ch = calc_chamfer_distance(xyz, pc, out=False)
            d1, d2 = calc_point_to_point_plane_psnr(xyz, pc, out=False)
            quality["subpixel %s, hidden_points %s" % (sub or "off", "on" if hid else "off")] = dict(
                container=len(blob), trailer=(4 + len(cd["hidden_points"])) if hid else 0, carried=int(bc.hidden_carried[0]) if hid else 0,
                uncarried=int(bc.hidden_uncarried[0]) if hid else 0, chamfer=ch["mean"], f_score=ch["f_score"], d1_psnr=d1["psnr_mean"], d2_psnr=d2["psnr_mean"])
    out["example_bzip2"] = quality
    q = lambda sub, hid: quality["subpixel %s, hidden_points %s" % (sub, hid)]
    out["condition_holds"] = bool(all(q(s, "on")["chamfer"] < q(s, "off")["chamfer"] and q(s, "on")["uncarried"] == 0 for s in ("off", 2)))
    print(json.dumps(out))
    print("| run | container bytes | trailer bytes | carried | Chamfer (m) | F-score | D1 PSNR | D2 PSNR |\n|---|---|---|---|---|---|---|---|")
    for k_, v in quality.items():
        print("| %s | %d | %d | %d | %.5f | %.4f | %.2f | %.2f |" % (k_, v["container"], v["trailer"], v["carried"], v["chamfer"], v["f_score"], v["d1_psnr"], v["d2_psnr"]))
    for k_, v in ker.items():
        print("%-20s %.3f ms (%.3f - %.3f) per %d frames" % (k_, v["median"], v["min"], v["max"], B))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    return 0 if out["condition_holds"] else 1


if __name__ == "__main__":
    sys.exit(main())
