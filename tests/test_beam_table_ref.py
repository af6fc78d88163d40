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


def test_past_the_grid_reaches_every_second_trip_and_the_carried_queue():
    """The batch of BT.past_the_grid(), by the reference and the launch rules alone (tests/grid_caps.py): every loop of the three kernels
    makes a second trip, and the LDS queue of beams_pix_kernel goes through a drain of two turns, a drain that only the carried queue
    causes, and a non-empty tail behind the loop.  A point counts as queued only where the fast path refuses it by rule (column 0, depth 0
    or not finite, an exact elevation tie) and as certainly fast only where it was aimed so (a quarter cell, a fifth of the way to the
    midpoint, 1 .. 60 m)."""
    import grid_caps as GC
    c = BT.past_the_grid()
    va, H, W = c["va"], c["H"], c["W"]
    B, P = len(c["frames"]), H * W
    total = sum(f.shape[0] for f in c["frames"])
    assert [f.shape[0] for f in c["distinct"]] == [8191, 8191, 8191, 0] and all(c["frames"][b] is c["distinct"][b % 4] for b in range(B))
    assert total >= GC.BEAMS_PIX_CAP * GC.BEAMS_CHUNK + 131072 and total > GC.BEAMS_WRITE_CAP * GC.BEAMS_WRITE_THREADS
    assert GC.trips(total, GC.BEAMS_CHUNK, GC.BEAMS_PIX_CAP) >= 2 and GC.trips(total, GC.BEAMS_WRITE_THREADS, GC.BEAMS_WRITE_CAP) >= 2
    assert GC.fill_trips(B * P, GC.BEAMS_FILL_THREADS, GC.BEAMS_FILL_CAP) >= 2
    assert total < 2 ** 31 and total * 12 < 40e6                                # (the kernels' own limit; the data stays below 40 MB)
    mid32 = (np.sort(va)[:-1] * 0.5 + np.sort(va)[1:] * 0.5).astype(np.float32)
    queued, ties = [], 0
    for f, fast in zip(c["distinct"], c["aimed_fast"]):
        keep, row, col, depth = R.pixels(f, va, HFOV, W)
        el = R.atan2f(f[:, 2], np.sqrt(f[:, 0] ** 2 + f[:, 1] ** 2))
        tie = np.isin(el, mid32)
        q = ~keep | (col == 0) | (depth == 0) | tie
        assert not (q & fast).any() and fast.shape == q.shape
        ties += int(tie.sum())
        queued.append(q)
    assert ties >= 550 and queued[1][: BT.PAST_HEAD].all() and not queued[2].any()
    # ties in ordinary columns: most are the last point of their pixel, so a queue that loses one changes the image (the points at the seam
    # share 16 pixels per frame: losing one of those shows only if it is the frame's last in its pixel)
    seam = c["distinct"][1]
    keep, row, col, depth = R.pixels(seam, va, HFOV, W)
    pix = row * W + col
    last = np.zeros(seam.shape[0], bool)
    last[np.unique(pix[::-1], return_index=True)[1]] = True
    last = last[::-1]
    el = R.atan2f(seam[:, 2], np.sqrt(seam[:, 0] ** 2 + seam[:, 1] ** 2))
    shown = np.isin(el, mid32) & (col != 0) & last
    assert shown.sum() >= 300 and shown[: BT.PAST_HEAD].sum() >= 1, (int(shown[: BT.PAST_HEAD].sum()), int(shown.sum()))   # (of at most W - 3: one row)
    # the tie goes to the lower row, and the zero that ends the zero-last frame leaves its pixel empty behind real points
    k, r, _, _ = R.pixels(c["tie"][None], va, HFOV, W)
    d = np.abs(va - float(R.atan2f(c["tie"][2:3], np.sqrt(c["tie"][0:1] ** 2 + c["tie"][1:2] ** 2))[0]))
    assert (d == d.min()).sum() == 2 and d.min() == BT.PAST_TIE_HALF and r[0] == np.flatnonzero(d == d.min())[0]
    zl = c["distinct"][0]
    keep, row, col, depth = R.pixels(zl, va, HFOV, W)
    same = (row == row[-1]) & (col == col[-1])
    assert depth[-1] == 0 and col[-1] == 0 and same.sum() == BT.PAST_RUN + 1 and R.project(zl, va, HFOV, H, W)[row[-1], col[-1]] == 0
    assert R.project(zl[:-1], va, HFOV, H, W)[row[-1], col[-1]] == depth[-2] > 0
    which = c["which"]
    q_all = np.concatenate([queued[k] for k in which])
    maybe_all = np.concatenate([~c["aimed_fast"][k] for k in which])
    facts = GC.queue_facts(q_all, maybe_all, total, GC.BEAMS_CHUNK, GC.BEAMS_PIX_CAP, GC.BEAMS_THREADS)
    print("beams past the grid: B %d, total %d, grid %d, trips %d; chunks of a drain or more %d (up to %d turns), carried %d, tails %d"
          % (B, total, facts["grid"], facts["trips"], facts["full"].size, facts["full_n"], facts["carried"].size, facts["tail"].size))
    assert facts["grid"] == GC.BEAMS_PIX_CAP and facts["trips"] >= 2
    assert facts["full_n"] >= 2                               # a chunk of 512 or more: two turns of the `while`
    assert facts["carried"].size >= 1                         # chunks k and k + cap, each below a drain, together one
    assert facts["tail"].size >= 1                            # a queue that is not empty behind the last trip
    first, end = GC.pix_rows(total, int(facts["carried"][0]), 1)
    assert GC.BEAMS_PIX_CAP * GC.BEAMS_CHUNK <= first < end <= total
    # a drain of one turn per chunk (the `while` as an `if`) would lose points whose loss the image shows: in both trips
    lost = GC.single_turn_losses(q_all, total, GC.BEAMS_CHUNK, GC.BEAMS_PIX_CAP, GC.BEAMS_THREADS)
    offs = np.concatenate([[0], np.cumsum([f.shape[0] for f in c["frames"]])])
    want = [R.project(f, va, HFOV, H, W) for f in c["distinct"]]
    changed = {}
    for b in (1, 5, int(np.flatnonzero(which == 1)[-1])):           # seam frames: the first two, and the last one (its points lie past the cap)
        assert which[b] == 1
        gone = lost[offs[b]: offs[b + 1]]
        changed[b] = int((R.project(c["frames"][b][~gone], va, HFOV, H, W).view(np.uint32) != want[1].view(np.uint32)).sum())
    print("a single turn per chunk would lose %d points; pixels that change in frames %s" % (int(lost.sum()), changed))
    assert lost.sum() > 1000 and all(v >= 8 for v in changed.values()) and offs[max(changed)] >= GC.BEAMS_PIX_CAP * GC.BEAMS_CHUNK


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
