"""GPU: what the subpixel channel costs and what it buys, on the example sweep (tests/golden/example_64E.npz: 122 320
rows, 64 x 2000):
  * ops.subpixel_encode / subpixel_decode beside ops.intensity_encode / intensity_decode on the same rows, --frames copies resident in HBM
    (the owner pass is shared work; the codes add two exact atan2f per non-empty pixel);
  * for bits off, 1 .. 4 at accuracy 0.02 with bzip2: the container's bytes, and Chamfer distance, F-score, D1 / D2 PSNR of the decoded
    points (evaluate_metrics) against the ORIGINAL example points -- with the option off those are the pixels' centre rays.
    The condition checked: D1 PSNR and Chamfer at every bits are strictly better than with the option off, and monotone in bits.
Each time is the median of RUNS runs after a warm-up (min - max beside it); the compared items take turns inside one process.
Usage: python tools_dev/subpixel_times.py [--frames 256] [--json FILE]; exit status 1 when the condition does not hold."""
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

ACCURACY, BITS = 0.02, (1, 2, 3, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    T = build_dataset(lidar_type="Velodyne64E").PCTransformer
    xyz = np.load(os.path.join(GOLDEN, "example_64E.npz"))["xyz"]
    k = np.load(os.path.join(GOLDEN, "intensity_example_64E.npz"))["k"]
    one = np.ascontiguousarray(np.concatenate([xyz, (k.astype(np.float32) / np.float32(100))[:, None]], 1), dtype=np.float32)
    n, P = one.shape[0], T.H * T.W
    out = dict(points_per_frame=n, runs=RUNS, accuracy=ACCURACY)

    # 1. the kernels alone
    B = a.frames
    L = ops._lib.lib()
    rows = torch.from_numpy(one).to(dev).repeat(B, 1).contiguous()
    offs = torch.arange(B + 1, dtype=torch.int64, device=dev) * n
    ri = ops.project(rows, offs, T.geom)
    u8, i32 = (lambda *s: torch.empty(s, dtype=torch.uint8, device=dev)), (lambda *s: torch.empty(s, dtype=torch.int32, device=dev))
    s_int, s_sub = u8(L.rpcc_intensity_scratch_bytes(B, P)), u8(L.rpcc_subpixel_scratch_bytes(B, P))
    ipay, inb, iorph, spay, snb, sorph = u8(B, 8 + P), i32(B), i32(B), u8(B, 8 + 2 * P), i32(B), i32(B)
    seg = torch.where(ri != 0, 2, 1).to(torch.uint8)
    w, pts, st = torch.empty_like(ri), torch.empty((B, T.H, T.W, 3), dtype=torch.float32, device=dev), i32(B)
    tab = T.subpixel_tables()
    fns = dict(intensity_encode=lambda: ops.intensity_encode(rows, offs, T.geom, ri, 100.0, payload=ipay, nbytes=inb, orphans=iorph, scratch=s_int),
               intensity_decode=lambda: ops.intensity_decode(ipay, inb, seg, out=w, status=st))
    for bits in BITS:
        fns["subpixel_encode_%d" % bits] = lambda bits=bits: ops.subpixel_encode(rows, offs, T.geom, ri, bits, payload=spay, nbytes=snb, orphans=sorph, scratch=s_sub)
    fns["subpixel_decode_4"] = lambda: ops.subpixel_decode(spay, snb, seg, ri, tab, out=pts, status=st)      # (behind subpixel_encode_4 in every round)
    ker = turns(fns, lambda f: device_ms(f, 10))
    assert not iorph.any() and not sorph.any() and not st.any()
    out["kernels_ms"] = dict(frames=B, **ker, encode_over_intensity=ker["subpixel_encode_2"]["median"] / ker["intensity_encode"]["median"])
    del rows, ri, s_int, s_sub, ipay, spay, seg, w, pts
    torch.cuda.empty_cache()

    # 2. size and quality of the example container, bzip2, against the original points
    host = cu.BasicCompressor(method_name="bzip2")
    quality = {}
    for bits in (None,) + BITS:
        bc = pipeline.BatchCompressor(T, accuracy=ACCURACY, basic_compressor="bzip2", subpixel_bits=bits)
        blob = bc.compress([one[:, :3]])[0]
        cd = cu.unpack_bitstream(blob, subpixel=bits is not None)
        pc = decode_frame(cd, host, T, 100, 2 * ACCURACY, None, True, subpixel=bits is not None)[1]
        ch = calc_chamfer_distance(xyz, pc, out=False)
        d1, d2 = calc_point_to_point_plane_psnr(xyz, pc, out=False)
        quality["off" if bits is None else str(bits)] = dict(container=len(blob), trailer=(4 + len(cd["subpixel"])) if bits else 0, chamfer=ch["mean"],
                                                             f_score=ch["f_score"], d1_psnr=d1["psnr_mean"], d2_psnr=d2["psnr_mean"])
    out["example_bzip2"] = quality
    order = ["off"] + [str(b) for b in BITS]
    cham, d1s = [quality[k_]["chamfer"] for k_ in order], [quality[k_]["d1_psnr"] for k_ in order]
    out["condition_holds"] = bool(all(x > y for x, y in zip(cham, cham[1:])) and all(x < y for x, y in zip(d1s, d1s[1:])))
    print(json.dumps(out))
    print("| bits | container bytes | trailer bytes | Chamfer (m) | F-score | D1 PSNR | D2 PSNR |\n|---|---|---|---|---|---|---|")
    for k_ in order:
        q = quality[k_]
        print("| %s | %d | %d | %.5f | %.4f | %.2f | %.2f |" % (k_, q["container"], q["trailer"], q["chamfer"], q["f_score"], q["d1_psnr"], q["d2_psnr"]))
    for k_, v in ker.items():
        print("%-20s %.3f ms (%.3f - %.3f) per %d frames" % (k_, v["median"], v["min"], v["max"], B))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    return 0 if out["condition_holds"] else 1


if __name__ == "__main__":
    sys.exit(main())
