"""Writes tests/golden/intensity_example_64E.npz: the fourth column of the reference's example sweep (assets/example_data/example.bin, rows
(x, y, z, intensity) as stored) and the intensity payload the specification (tests/intensity_ref.py) gives for it at scale 100.

Stored: k uint8 [N] with intensity == fl(k / 100) bit for bit (asserted here), and payload uint8 [8 + n].  The points themselves are the
xyz of tests/golden/example_64E.npz, which equal the stored rows (asserted here).  Runs only where the reference tree exists; it reads the
sweep as data, none of the reference's program text is used.

Run from the repository root: python tests/golden/gen_golden_intensity.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import intensity_ref as R  # noqa: E402
from oracle import oracle as orc  # noqa: E402

SWEEP = "/root/reference/assets/example_data/example.bin"


def main():
    rows = np.fromfile(SWEEP, dtype=np.float32).reshape(-1, 4)
    xyz = np.load(os.path.join(HERE, "example_64E.npz"))["xyz"]
    assert np.array_equal(rows[:, :3].view(np.uint32), xyz.view(np.uint32)), "example_64E.npz does not hold the stored rows"
    k = np.rint(rows[:, 3].astype(np.float64) * 100)
    assert k.min() >= 0 and k.max() <= 255
    k = k.astype(np.uint8)
    w = k.astype(np.float32) / np.float32(100)
    assert np.array_equal(w.view(np.uint32), rows[:, 3].view(np.uint32)), "the intensities are not fl(k / 100)"
    g = orc.LidarGeom(**orc.GEOMS["Velodyne64E"])
    e = R.encode_frame(rows, g, 100)
    assert np.array_equal(R.owners_closed(e["d"], e["pix"], e["ri"]), e["own"])
    assert np.array_equal(R.dequantise(e["q"], 100).view(np.uint32), rows[e["own"][e["ri"] != 0], 3].view(np.uint32)), "scale 100 is not lossless"
    out = os.path.join(HERE, "intensity_example_64E.npz")
    np.savez_compressed(out, k=k, payload=e["payload"])
    print("%s: %d points, k = %d .. %d, %d non-empty pixels, %d bytes" % (out, k.shape[0], k.min(), k.max(), e["q"].shape[0], os.path.getsize(out)))


if __name__ == "__main__":
    main()
