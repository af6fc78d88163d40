"""The facts the generators of tests/filter_cases.py claim about their cases, asserted on the CPU with the numpy reference
(tests/radius_filter_ref.py): what tests/test_gpu_radius_filter.py runs on the device exercises what it is meant to.  No GPU needed."""
import numpy as np
import pytest

import filter_cases as FC
import radius_filter_ref as R


def ref(case):
    xyz, offsets, nb_points, radius = case
    return R.radius_filter(xyz, offsets, nb_points, radius)


@pytest.mark.parametrize("n", FC.FRAME_SIZES)
def test_single_frames(n):
    case, f = FC.single_frame(n)
    assert case[0].shape == (n, 3) and f["tiles"] == -(-n // 256)
    keep = ref(case)["keep"]
    if n > 1:
        assert keep.any() and not keep.all()      # both answers occur
        assert np.array_equal(R.frame_counts(case[0], 1.0), R.brute_counts(case[0], 1.0))
    else:
        assert not keep.any()                     # a single point has one neighbour, itself


def test_mixed_batch_is_cut_per_frame():
    case, f = FC.mixed_batch()
    xyz, offsets, nb, radius = case
    assert offsets.tolist() == [0, 300, 300, 557, 558] and f["tiles"] == 2 + 0 + 2 + 1
    tile, T = FC.tile_of(offsets)
    assert T == 5 and tile[299] == 1 and tile[300] == 2      # a global cut every 256 points would put 256 .. 511 into one tile
    per_frame = ref(case)
    merged = R.radius_filter(xyz, None, nb, radius)
    assert not np.array_equal(per_frame["count"], merged["count"])      # the frames overlap: isolation shows
    assert per_frame["kept"][1] == 0 and per_frame["kept"][3] == 0


def test_twin_frames_meet_at_the_border():
    case, f = FC.twin_frames()
    xyz, offsets, nb, radius = case
    tw = f["twins"]
    assert tw[-1] == offsets[1] and tw[-2] == offsets[1] - 1 and np.all(xyz[tw] == xyz[tw[0]])
    assert not ref(case)["keep"][tw].any()
    assert R.radius_filter(xyz, None, nb, radius)["keep"][tw].all()
    assert ref(case)["kept"].tolist() == [nb + 1, nb + 1]


@pytest.mark.parametrize("nb", FC.THRESHOLD_NB)
def test_threshold_groups(nb):
    case, f = FC.threshold_groups(nb)
    xyz = case[0]
    g = f["groups"]
    full = R.frame_counts(xyz, case[3])
    assert np.array_equal(full, R.brute_counts(xyz, case[3]))
    for name, pos in g.items():
        assert len(pos) == f["sizes"][name] and np.all(full[pos] == len(pos)), name      # every member sees exactly its group
    members = np.concatenate(list(g.values()))
    assert len(set(members.tolist())) == members.size
    filler = np.setdiff1d(np.arange(xyz.shape[0]), members)
    assert np.all(full[filler] == 1)
    keep = ref(case)["keep"]
    assert not keep[g["below"]].any() and keep[g["at"]].all()
    assert keep[g["dup"]].all() and np.all(xyz[g["dup"]] == xyz[g["dup"][0]]) and len(g["dup"]) == 60
    assert f["spread_tiles"] == [0, 1, 3] and keep[g["spread"]].all()
    own = np.array([np.count_nonzero(g["spread"] // 256 == p // 256) for p in g["spread"]])
    assert np.all(own <= nb) or nb == 0      # no member of the spread group is kept by its own tile alone
    assert keep[filler].all() == (nb == 0)


@pytest.mark.parametrize("radius", FC.BAND_RADII)
def test_band_pairs(radius):
    case, f = FC.band_pairs(radius)
    gs = f["groups"]
    lo, hi = FC.screen_bounds(radius)
    assert lo < np.float32(radius * radius) < hi and (f["lo"], f["hi"]) == (lo, hi)
    assert all(lo <= g["d2f"] <= hi for g in gs)                          # every pair gets the exact test ...
    edge = [g for g in gs if not g["in_band"]]                            # ... strictly inside the band, but for radius 1.0, step +3 (one per axis):
    assert len(edge) == (3 if radius == 1.0 else 0)                       # d2f == hi, the last value the screen passes on to the exact test
    assert all(g["step"] == 3 and g["d2f"] == hi for g in edge)
    assert any(g["in_band"] and g["neighbour"] for g in gs) and any(g["in_band"] and not g["neighbour"] for g in gs)
    assert any(g["neighbour"] for g in gs) and not all(g["neighbour"] for g in gs)      # both sides of the fp64 decision
    assert sorted({g["step"] for g in gs}) == list(FC.BAND_STEPS)
    planted = [g for g in gs if g["planted"]]
    assert bool(planted) == f["exact_planted"] and all(not g["neighbour"] and g["step"] == 0 for g in planted)
    if radius == 1.0:
        assert len(planted) == 3
    want = FC.band_expected(case, f)
    assert np.array_equal(ref(case)["keep"], want)
    tile, _ = FC.tile_of(case[1])
    assert any(tile[g["partner"]] != tile[g["copies"][0]] for g in gs)


def test_band_pairs_hold_a_pair_fp32_alone_would_misjudge():
    """A pair that d2_f32 < float32(r^2) would decide the other way than the fp64 rule, at three radii of the set."""
    wrong = {r: sum(g["fp32_neighbour"] != g["neighbour"] for g in FC.band_pairs(r)[1]["groups"]) for r in FC.BAND_RADII}
    assert wrong[0.45] > 0 and wrong[1.0] > 0 and wrong[6.0] > 0, wrong


def test_far_tiles():
    case, f = FC.far_tiles()
    xyz, offsets, nb, radius = case
    assert f["tiles"] > FC.TILE_LIST and xyz.shape[0] == f["n"] and f["n"] % 256 != 0
    tile, T = FC.tile_of(offsets)
    assert T == f["tiles"]
    loners = f["loners"]
    assert np.all(tile[loners[:-1]] == 0) and tile[loners[-1]] == T - 1 and T - 1 >= FC.TILE_LIST      # the partner: last, partial tile, second round
    r = ref(case)
    assert r["keep"][loners].all() and np.all(r["count"][loners] == nb + 1)
    cut = R.radius_filter(xyz[:(T - 1) * 256], None, nb, radius)
    assert not cut["keep"][loners[:-1]].any()                              # without the last tile the copies are removed
    assert not r["keep"][f["outlier"]] and r["count"][f["outlier"]] == 1
    lo, hi, cnt = FC.tile_boxes(xyz, offsets)
    q = xyz[f["outlier"]][None]
    assert np.all(FC.box_bound(q, q, lo, hi) == 0)                         # every tile passes the outlier's box filter
    q0lo, q0hi = lo[:1], hi[:1]
    assert np.count_nonzero(FC.box_bound(q0lo, q0hi, lo, hi) <= FC.screen_bounds(radius)[1]) == T      # and fills the list of tile 0
    assert int((~r["keep"]).sum()) < 50                                    # the scene is dense: nearly everything else is kept


def test_nonfinite():
    case, f = FC.nonfinite()
    xyz, offsets, nb, radius = case
    assert xyz.shape[1] == 4 and xyz.shape[0] <= 256
    bad = xyz[f["bad"], :3]
    assert len(bad) == 9 and np.all((~np.isfinite(bad)).sum(1) == 1)
    for axis in range(3):
        col = bad[~np.isfinite(bad[:, axis]), axis]
        assert np.isnan(col).sum() == 1 and (col == np.inf).sum() == 1 and (col == -np.inf).sum() == 1
    r = ref(case)
    assert not r["keep"][f["bad"]].any() and np.all(r["count"][f["bad"]] == 0)
    assert not r["keep"][f["A"]].any() and np.all(r["count"][f["A"]] == nb)      # the bad points are invisible
    repaired = xyz.copy()
    repaired[f["bad"], :3] = xyz[f["A"][0], :3]
    assert R.radius_filter(repaired, offsets, nb, radius)["keep"][f["A"]].all()  # ... and would have decided otherwise
    assert r["keep"][f["B"]].all() and np.isnan(xyz[f["B"], 3]).sum() == 2
    lo, hi, cnt = FC.tile_boxes(xyz, offsets)
    assert np.isfinite(lo).all() and np.isfinite(hi).all() and cnt[0] == xyz.shape[0] - 9


def test_sweep_slices_and_order():
    sl = FC.sweep_slices()
    assert sorted(sl) == ["beams", "columns"]
    for name, xyz in sl.items():
        assert 2000 <= xyz.shape[0] <= 9000, (name, xyz.shape)
        a, b, perm = FC.ordered_and_shuffled(xyz)
        ra, rb = ref(a), ref(b)
        assert np.array_equal(ra["keep"][perm], rb["keep"])
        assert ra["keep"].any() and not ra["keep"].all(), name


def test_golden_of_the_example_sweep():
    g = FC.golden()
    xyz = FC.example_sweep()
    assert g["n"] == xyz.shape[0] == 122320 and g["removed"].size == 283
    assert np.array_equal(np.nonzero(~g["keep"])[0], g["removed"])
    r = R.radius_filter(xyz, None, 3, 1.0)
    assert np.array_equal(r["keep"], g["keep"])
    assert g["boundary_pairs"].shape == (1, 2)      # the sweep holds one pair at d^2 == r^2 (millimetre coordinates, 1.000 m apart along x)
    i, j = g["boundary_pairs"][0]
    assert R.d2(xyz[i].astype(np.float64), xyz[j].astype(np.float64)) == 1.0 and g["keep"][i] and g["keep"][j]
