"""Writes tests/golden/radius_filter_example_64E.npz: the radius outlier removal of the example sweep (example_64E.npz, stored order)
at nb_points = 3, radius = 1.0 by the numpy reference (tests/radius_filter_ref.py): the packed keep bits, the removed indices, and
the pairs whose fp64 d^2 lies within 4 fp64 ulps of r^2.

The sweep holds such a pair (KITTI coordinates are millimetres: two points differ by exactly 1.000 m along x), so the golden does
not claim that there is none; it asserts what makes it independent of the boundary rule all the same: every point of such a pair is
kept whether or not its partner counts.  Against scipy's cKDTree (<= at the boundary) the counts agree on every other point.

Run from the repository root: python tests/golden/gen_golden_radius_filter.py (needs scipy)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import radius_filter_ref as R  # noqa: E402

NB_POINTS, RADIUS = 3, 1.0


def main():
    from scipy.spatial import cKDTree
    xyz = np.load(os.path.join(HERE, "example_64E.npz"))["xyz"].astype(np.float32)
    ref = R.radius_filter(xyz, None, NB_POINTS, RADIUS, full=True)
    pairs = R.near_boundary(xyz, RADIUS, ulps=4)
    touched = np.unique(pairs)
    assert np.all(ref["full"][touched] - np.bincount(pairs.reshape(-1), minlength=xyz.shape[0])[touched] > NB_POINTS), \
        "a point near the boundary is kept or removed by the boundary rule"
    p64 = xyz.astype(np.float64)
    tree = cKDTree(p64).query_ball_point(p64, RADIUS, return_length=True, workers=-1)
    other = np.setdiff1d(np.arange(xyz.shape[0]), touched)
    assert np.array_equal(tree[other], ref["full"][other]), "the reference and cKDTree disagree away from the boundary"
    assert np.array_equal(tree > NB_POINTS, ref["keep"])
    capped = R.radius_filter(xyz, None, NB_POINTS, RADIUS)
    assert np.array_equal(capped["keep"], ref["keep"]) and np.array_equal(capped["count"], ref["count"])
    removed = np.nonzero(~ref["keep"])[0].astype(np.int64)
    np.savez_compressed(os.path.join(HERE, "radius_filter_example_64E.npz"), keep_bits=np.packbits(ref["keep"]), removed=removed,
                        n=np.int64(xyz.shape[0]), nb_points=np.int64(NB_POINTS), radius=np.float64(RADIUS), boundary_pairs=pairs)
    print("%d points, %d removed, %d boundary pairs" % (xyz.shape[0], removed.size, pairs.shape[0]))


if __name__ == "__main__":
    main()
