"""Generates tests/golden/dbscan_example_64E.npz: the final DBSCAN seg_idx of the real 64-beam sweep (example_64E.npz,
ground plane injected from its ground_model), computed by sklearn's DBSCAN -- an implementation independent of both the
kernels and tests/dbscan_ref.py -- with the reference's relabelling (utils/segment_utils.py:149-169).

sklearn counts neighbours with d <= eps, the specification with d < eps: the generator asserts that no candidate pair of
the frame sits at exactly d^2 == eps^2 in fp64, so the two rules give the same clusters here.

    python tests/golden/gen_golden_dbscan.py        (needs sklearn; run from the repository root)"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

EPS, MIN_POINTS = 1.5, 10


def main():
    from oracle import oracle as orc
    import dbscan_ref as R
    z = np.load(os.path.join(HERE, "example_64E.npz"))
    g = orc.LidarGeom(**orc.GEOMS["Velodyne64E"])
    tm = orc.transform_map(g)
    ri = orc.project(z["xyz"], g)
    gm = z["ground_model"]
    # no pair at the boundary: real-real candidates from the grid, and every real point against the origin
    ng = R.nonground(ri, tm, gm)
    pts = R.points(ri, tm)[ng & (ri != 0)].astype(np.float64)
    grid = R._Grid(pts, EPS)
    e2 = EPS * EPS
    for c0 in range(0, len(pts), R.CHUNK):
        q, c = grid.pairs(np.arange(c0, min(len(pts), c0 + R.CHUNK)))
        assert not np.any(R.d2(pts[q], pts[c]) == e2), "a pair at d^2 == eps^2: sklearn's <= would differ"
    assert not np.any(R.d2(pts, np.zeros(3)) == e2)
    seg = R.sklearn_labels(ri, tm, gm, EPS, MIN_POINTS)
    out = os.path.join(HERE, "dbscan_example_64E.npz")
    np.savez_compressed(out, seg_idx=seg.astype(np.int16), eps=np.float64(EPS), min_points=np.int32(MIN_POINTS))
    print("wrote %s: labels 0..%d, %d non-ground points" % (out, int(seg.max()), int(ng.sum())))


if __name__ == "__main__":
    main()
