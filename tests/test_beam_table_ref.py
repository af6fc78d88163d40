"""The specification of the per-beam table projection (tests/beam_table_ref.py) without a GPU: against an explicit per-point loop on
constructed points, against the genuine reference's table branch on the example sweep (tests/golden/beam_table_example_64E.npz, written by
tests/golden/gen_golden_beam_table.py), the table-built transform map against the reference's formula, and the rule that separates it from
the even projection (the last point wins, not the nearest)."""
import math
import os

import numpy as np
import pytest

import beam_table_cases as BT
import beam_table_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSV = os.path.join(ROOT, "r-pcc_amd", "lidar_cfg", "Velodyne_HDL_64E_beams.csv")
HFOV = 360 * (np.pi / 180)


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as ge
    ge.build()


def ray(az, el, r=10.0):
    return [r * math.cos(el) * math.cos(az), r * math.cos(el) * math.sin(az), r * math.sin(el)]


def constructed(va, W, seed=0):
    """A few hundred points: random ones, runs on one pixel, columns at halves / 0 / W, a trailing depth-0 point, non-finite points."""
    rng = np.random.default_rng(seed)
    lo, hi = float(np.min(va)) - 0.05, float(np.max(va)) + 0.05
    pts = [ray(a, e, r) for a, e, r in zip(rng.uniform(0, 2 * np.pi, 300), rng.uniform(lo, hi, 300), rng.uniform(1, 60, 300))]
    step = 2 * np.pi / W
    for k in (0.5, 1.5, 2.5, W - 0.5, W - 0.49, 0.0, W - 1e-4):       # halves to even and odd neighbours, column 0, rounding to W -> 0
        pts.append(ray(k * step, float(va[0]), 7.0))
    pts += [ray(1.0, float(va[-1]), r) for r in (3.0, 9.0, 5.0)]      # one pixel: the nearest first, the last one stays
    pts += [[0.0, 0.0, 0.0], ray(2.0, float(va[0]), 4.0), [0.0, 0.0, 0.0]]   # depth 0 in the middle of its pixel's run and last
    pts += [[np.nan, 1, 1], [np.inf, 0, 0], [3e19, 3e19, 1.0], [1, -np.inf, 2], ray(2.5, lo - 0.3), ray(2.5, hi + 0.3)]
    pts += [[5.0, -0.0, 0.1], [5.0, -1e-30, 0.1], [-5.0, -1e-30, 0.1]]     # az = -0.0, tiny negative az
    pts.append(ray(0.3, float(va[0]), 2.0))
    return np.array(pts, dtype=np.float32)


TABLES = {
    "ascending": np.radians(np.linspace(-24.0, 2.0, 5)),
    "descending": np.radians(np.linspace(2.0, -24.0, 5)),
    "shuffled": np.radians([-3.0, 1.5, -20.0, -11.0, -7.5, 0.25]),
    "duplicates": np.radians([-10.0, -2.0, -10.0, -2.0, 1.0]),
    "single": np.radians([-5.0]),
    "two": np.radians([1.0, -9.0]),
}


@pytest.mark.parametrize("name", sorted(TABLES))
@pytest.mark.parametrize("W", (8, 64))
def test_specification_equals_the_loop(name, W):
    va = TABLES[name]
    H = len(va)
    xyz = constructed(va, W, seed=W + H)
    assert np.array_equal(R.project(xyz, va, HFOV, H, W).view(np.uint32), R.project_loop(xyz, va, HFOV, H, W).view(np.uint32))


def test_rules_on_hand_made_points():
    va = np.radians([0.0, 10.0, 0.0, -10.0])            # rows 0 and 2 are equal: row 0 takes their points
    H, W = 4, 8
    step = 2 * np.pi / W
    # an exact fp64 tie between two entries: the first one in ROW order, whichever is the larger angle
    p = np.array([[math.cos(0.5), 0.0, math.sin(0.5)]], dtype=np.float32)
    el = R.atan2f(p[:, 2], np.sqrt(p[:, 0] ** 2 + p[:, 1] ** 2))[0]
    tie2 = np.array([float(el) + 0.25, float(el) - 0.25])
    keep, row, col, _ = R.pixels(p, tie2, HFOV, W)
    assert keep[0] and row[0] == 0 and abs(tie2[0] - float(el)) == abs(tie2[1] - float(el))
    keep, row, col, _ = R.pixels(p, tie2[::-1].copy(), HFOV, W)
    assert row[0] == 0
    # equal entries -> the lowest row; last wins; a trailing depth-0 point leaves 0; non-finite points are skipped
    xyz = np.array([ray(step, 0.0, 3.0), ray(step, 0.0, 9.0), ray(step, 0.0, 5.0),
                    ray(3 * step, math.radians(10), 4.0), [0, 0, 0],
                    [np.nan, 0, 0], ray(2 * step, math.radians(-10), 6.0), [np.inf, 1, 1]], dtype=np.float32)
    ri = R.project(xyz, va, HFOV, H, W)
    assert ri[0, 1] == np.float32(np.sqrt(np.float32(xyz[2, 0] ** 2 + xyz[2, 1] ** 2) + xyz[2, 2] ** 2)) and abs(ri[0, 1] - 5.0) < 1e-5
    assert ri[2].max() == 0                               # the second of two equal rows stays empty
    assert ri[0, 0] == 0 and abs(ri[1, 3] - 4.0) < 1e-5 and abs(ri[3, 2] - 6.0) < 1e-5
    assert np.count_nonzero(ri) == 3
    xyz2 = np.concatenate([xyz, np.array([ray(0.0, 0.0, 2.0), [0, 0, 0]], dtype=np.float32)])
    assert R.project(xyz2, va, HFOV, H, W)[0, 0] == 0     # (0,0,0) comes last on pixel (0, 0)
    # half to even and the wrap W -> 0
    for k, want in ((0.5, 0), (1.5, 2), (2.5, 2), (W - 0.5, 0), (W - 0.2, 0)):
        colf = np.float32(np.float32(k * step) / np.float32(HFOV) * np.float32(W))
        if abs(float(colf) - k) < 1e-9:                   # (the product is exactly the half only where fp32 allows)
            assert int(np.rint(colf)) % W == want


def test_specification_equals_the_genuine_reference():
    g = np.load(os.path.join(HERE, "golden", "beam_table_example_64E.npz"))
    xyz = np.load(os.path.join(HERE, "golden", "example_64E.npz"))["xyz"].astype(np.float32)
    va = R.read_csv(CSV)
    assert np.array_equal(va, g["vertical_angle"]) and va.shape == (64,)
    keep, row, col, _ = R.pixels(xyz, va, HFOV, 2000)
    assert keep.all() and np.array_equal(row, g["row"]) and np.array_equal(col, g["col"])
    ri = R.project(xyz, va, HFOV, 64, 2000)
    assert np.array_equal(ri.view(np.uint32), g["ri"].view(np.uint32))
    # what makes this its own projection: in thousands of pixels the last point is not the nearest, so the min-depth rule fails the golden
    pix = row * 2000 + col
    depth = np.sqrt((xyz * xyz).sum(1, dtype=np.float32)).astype(np.float32)
    mind = np.full(64 * 2000, np.inf, dtype=np.float32)
    np.minimum.at(mind, pix, depth)
    touched = np.unique(pix)
    assert int((mind[touched] != g["ri"].reshape(-1)[touched]).sum()) > 1000


def test_shipped_csv_is_the_nominal_layout():
    import csv
    rows = list(csv.DictReader(open(CSV)))
    assert [int(r["channel"]) for r in rows] == list(range(64))
    deg = np.array([float(r["vertical_angle"]) for r in rows])
    assert np.all(np.diff(deg) > 0) and deg[0] == -24.33 and deg[31] == -8.83 and deg[32] == -8.33 and deg[63] == 2.0
    assert np.allclose(np.diff(deg[:32]), 0.5, atol=1e-4) and np.allclose(np.diff(deg[32:]), 10.33 / 31, atol=1e-4)


def test_transform_map_from_the_table():
    import rpcc_amd  # noqa: F401
    from rpcc_amd import ops
    va = R.read_csv(CSV)
    for H, W, v in ((64, 2000, va), (5, 16, TABLES["descending"]), (6, 8, TABLES["shuffled"])):
        tm = ops.transform_map(H, W, HFOV, 0.1, -0.4, vertical_angle=v)
        assert tm.dtype == np.float32 and np.array_equal(tm.view(np.uint32), R.transform_map(v, HFOV, H, W).view(np.uint32))
    even = ops.transform_map(64, 2000, HFOV, 2.0 * (np.pi / 180), -24.9 * (np.pi / 180))
    assert not np.array_equal(even, ops.transform_map(64, 2000, HFOV, 0.0, 0.0, vertical_angle=va))
    # the genuine reference's table-built map (its bytes' sha256, stored by the golden's generator)
    import hashlib
    g = np.load(os.path.join(HERE, "golden", "beam_table_example_64E.npz"))
    tm = ops.transform_map(64, 2000, HFOV, 0.0, 0.0, vertical_angle=va)
    assert hashlib.sha256(tm.tobytes()).digest() == g["transform_map_sha256"].tobytes()
    assert hashlib.sha256(R.transform_map(va, HFOV, 64, 2000).tobytes()).digest() == g["transform_map_sha256"].tobytes()


@pytest.mark.parametrize("W", (8, 64))
@pytest.mark.parametrize("H", (2, 5))
def test_constructed_sets_reach_what_they_aim_at(H, W):
    """The GPU tests' constructed sets (tests/beam_table_cases.py), every table: elevations AT each float32 midpoint of sorted neighbours and at
    the two float32 values on either side; pre-rounding columns at exact halves with even and odd neighbours, at 0 and at W."""
    for name, (va, tie) in BT.tables(H).items():
        xyz = BT.constructed(va, W, tie)
        with np.errstate(all="ignore"):
            el = R.atan2f(xyz[:, 2], np.sqrt(xyz[:, 0] ** 2 + xyz[:, 1] ** 2))
            az = R.atan2f(xyz[:, 1], xyz[:, 0])
            az = np.where(az < 0, az + R.TWO_PI_F, az).astype(np.float32)
            colf = az / np.float32(HFOV) * np.float32(W)
        s = np.sort(va)
        for m in (s[:-1] * 0.5 + s[1:] * 0.5).astype(np.float32):
            for d in (-2, -1, 0, 1, 2):
                t = m
                for _ in range(abs(d)):
                    t = np.nextafter(t, np.float32(np.inf if d > 0 else -np.inf))
                assert (el == t).any(), (name, m, d)
        for k in (0.5, 1.5, 2.5, W - 0.5):
            assert (colf == np.float32(k)).any(), (name, k)
        assert (colf == 0).any() and (colf == W).any(), name
