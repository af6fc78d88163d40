"""The facts the generators of tests/tile_cases.py claim about themselves, asserted on the CPU (so a case cannot silently stop
exercising what it is for), and the numpy references against sklearn / cKDTree on those cases where the libraries are
installed.  The device runs the cases in tests/test_gpu_tile_search.py."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import dbscan_ref as R   # noqa: E402
import eval_ref as E     # noqa: E402
import tile_cases as C   # noqa: E402


# ------------------------------------------------------------------------------------------------
# folded
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def folded_frames():
    return {s: C.folded(*s) for s in C.FOLDED_SHAPES}


def test_folded_shapes(folded_frames):
    f = folded_frames[(2048, 160)][1]
    assert f["T"] == 1280 > C.TILE_LIST and 2048 > C.SCAN_CHUNK and f["real"] == 15360 and f["zero"] > 0
    f = folded_frames[(72, 4096)][1]
    assert f["T"] == 1152 > C.TILE_LIST and not f["rows"] and f["real"] <= C.MAX_REAL and f["zero"] > 0
    assert 72 % C.TILE_R == 0 and 160 % C.TILE_C == 0


@pytest.mark.parametrize("shape", C.FOLDED_SHAPES)
def test_folded_depends_on_second_round(folded_frames, shape):
    """For every parameter pair used with it, the reference labels of pixels in tiles < 1024 change when every pixel of a tile
    >= 1024 is turned into ground; the second pair has the larger eps."""
    (ri, tm, g), f = folded_frames[shape]
    low = C.tile_index(*shape) < C.TILE_LIST
    ri2, tm2 = C.cut_high_tiles(ri, tm)
    assert np.array_equal(ri[low], ri2[low]) and np.array_equal(tm[low], tm2[low]) and not R.nonground(ri2, tm2, g)[~low].any()
    assert len(f["params"]) == 2 and f["params"][1][0] > f["params"][0][0]
    for eps, mp in f["params"]:
        full, part = R.dbscan_frame(ri, tm, g, eps, mp), R.dbscan_frame(ri2, tm2, g, eps, mp)
        assert int((full[low] != part[low]).sum()) >= 30, (eps, mp)
        assert max(full.max(), part.max()) >= 4       # several clusters, with or without the far tiles
    if shape == (2048, 160):
        eps, mp = f["params"][0]
        assert (eps, mp) == (0.45, 6)
        full, part = R.dbscan_frame(ri, tm, g, eps, mp), R.dbscan_frame(ri2, tm2, g, eps, mp)
        assert int((full[low] != part[low]).sum()) == 2868


@pytest.mark.parametrize("shape", C.FOLDED_SHAPES)
def test_folded_eval_nearest_crosses_the_list(shape):
    (p1, p2), f = C.folded_eval(*shape)
    a, b = E.compact(p1), E.compact(p2)
    assert (a.shape[0], b.shape[0]) == (f["n1"], f["n2"]) and f["n2"] < f["n1"]
    _, i12 = E.nn(a, b)
    assert C.nn_crossings(p1, p2, i12) >= 100
    _, i21 = E.nn(b, a)
    assert np.array_equal(a[i21], b)   # cloud 2 is a subset of cloud 1: every point finds itself


def test_second_frame_differs(folded_frames):
    (ri, tm, g), _ = folded_frames[(2048, 160)]
    ri2 = C.second_frame(ri, tm)
    assert int((ri2 == 2).sum()) > 1000 and int(((ri2 == 0) & (ri != 0)).sum()) == 25
    eps, mp = C.FOLDED_PARAMS[(2048, 160)][0]
    assert not np.array_equal(R.dbscan_frame(ri, tm, g, eps, mp), R.dbscan_frame(ri2, tm, g, eps, mp))


# ------------------------------------------------------------------------------------------------
# scattered
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,n", C.SCATTERED_SHAPES)
def test_scattered_fills_the_list(H, W, n):
    (ri, tm, g), f = C.scattered(H, W, n)
    want_T = {(2048, 160): 1280, (8, 32768): 1024, (8, 32769): 1025}[(H, W)]
    assert f["T"] == want_T == C.tile_count(H, W) and f["real"] == n <= C.MAX_REAL
    if W == 32769:   # the last tile is one column wide
        assert np.count_nonzero(C.tile_index(H, W) == 1024) == H
    for eps, _ in f["params"]:
        frac, nonempty = C.scattered_fill(ri, tm, eps)
        assert nonempty >= min(f["T"], 1024) and frac >= 0.9, (eps, frac, nonempty)
    # the anchor copies: one in the last tile, the others in tile 0; core at the largest min_points only with all of them
    tile = C.tile_index(H, W).reshape(-1)
    assert tile[f["anchor"][0]] == f["T"] - 1 and (tile[f["anchor"][1:]] == 0).all()
    eps, mp = max(f["params"], key=lambda e: e[1])
    assert f["anchor"].size == mp
    full = R.dbscan_frame(ri, tm, g, eps, mp).reshape(-1)
    ri2, tm2 = C.cut_high_tiles(ri, tm, first=f["T"] - 1)
    part = R.dbscan_frame(ri2, tm2, g, eps, mp).reshape(-1)
    assert (full[f["anchor"]] >= 3).all() and (part[f["anchor"][1:]] == 2).all()
    (p1, p2), fe = C.scattered_eval(H, W, n)
    a, b = E.compact(p1), E.compact(p2)
    assert (a.shape[0], b.shape[0]) == (fe["n1"], fe["n2"])
    d, i = E.nn(a[:1], b)
    assert d[0] == 0 and i[0] == fe["n2"] - 1 and np.array_equal(p2[H - 1, W - 1], a[0])   # the anchor's answer: the last tile


def test_box_bound_is_a_lower_bound():
    """The numpy box_bound is what the claim above rests on: never above the fp32 distance of any pair of the two boxes."""
    rng = np.random.default_rng(0)
    a, b = rng.uniform(-5, 5, (40, 6, 3)).astype(np.float32), rng.uniform(-5, 5, (50, 7, 3)).astype(np.float32)
    bb = C.box_bound(a.min(1), a.max(1), b.min(1), b.max(1))
    for i in range(40):
        for j in range(50):
            assert bb[i, j] <= C.d2f(a[i][:, None], b[j][None]).min()
    assert (bb > 0).any() and (bb == 0).any()


# ------------------------------------------------------------------------------------------------
# small shapes
# ------------------------------------------------------------------------------------------------
def test_small_shapes_cover_partial_tiles():
    cases = C.small_shapes()
    assert [(f["H"], f["W"]) for _, _, f in cases] == list(C.SMALL_SHAPES)
    assert any(f["partial_rows"] and f["second_scan_chunk"] for _, _, f in cases)
    assert any(f["partial_rows"] and not f["partial_cols"] for _, _, f in cases)
    assert any(f["partial_cols"] and f["H"] == 1 for _, _, f in cases)
    for (ri, tm, g), (p1, p2), f in cases:
        assert f["real"] == int(C.real_mask(ri, tm).sum()) and ri.shape == (f["H"], f["W"])
        assert (E.compact(p1).shape[0], E.compact(p2).shape[0]) == (f["n1"], f["n2"])
    # not trivial: clusters exist on the larger shapes
    (ri, tm, g), _, f = cases[-1]
    assert R.dbscan_frame(ri, tm, g, *f["params"][0]).max() >= 4


# ------------------------------------------------------------------------------------------------
# sweep
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sweep_results():
    out = {}
    for seed in C.SWEEP_SEEDS:
        (ri, tm, g), f = C.sweep_cloud(seed)
        for eps in f["eps"]:
            for mp in f["min_points"]:
                out[(seed, eps, mp)] = R.dbscan_frame(ri, tm, g, eps, mp, with_clusters=True)
    return out


def test_sweep_covers_the_outcomes(sweep_results):
    kinds = set()
    for (seed, eps, mp), (seg, cl, core) in sweep_results.items():
        (ri, tm, g), f = C.sweep_cloud(seed)
        ncl = int(cl.max()) + 1 if cl.size else 0
        if ncl == 0:
            kinds.add("all_noise")
        if ncl == 1 and not (seg == 2).any():
            kinds.add("single_cluster")
        if ncl > 20:
            kinds.add("many_clusters")
        ng = R.nonground(ri, tm, g).reshape(-1)
        origin = ri.reshape(-1)[ng] == 0
        assert origin.sum() > 0
        kinds.add("origin_core" if core[np.argmax(origin)] else "origin_not_core")
    assert kinds == {"all_noise", "single_cluster", "many_clusters", "origin_core", "origin_not_core"}
    shapes = set(C.SWEEP_SEEDS.values())
    assert shapes == {(16, 128), (64, 512)}


def test_sweep_reference_against_sklearn(sweep_results):
    pytest.importorskip("sklearn")
    for (seed, eps, mp), (seg, _, _) in sweep_results.items():
        (ri, tm, g), _ = C.sweep_cloud(seed)
        assert not C.has_exact_pair(ri, tm, eps)
        assert np.array_equal(seg, R.sklearn_labels(ri, tm, g, eps, mp)), (seed, eps, mp)


def test_small_and_folded_reference_against_sklearn(folded_frames):
    pytest.importorskip("sklearn")
    for (ri, tm, g), _, f in C.small_shapes():
        for eps, mp in f["params"]:
            assert not C.has_exact_pair(ri, tm, eps)
            assert np.array_equal(R.dbscan_frame(ri, tm, g, eps, mp), R.sklearn_labels(ri, tm, g, eps, mp)), (f["H"], f["W"], eps, mp)
    for shape, ((ri, tm, g), f) in folded_frames.items():
        for eps, mp in f["params"]:
            assert np.array_equal(R.dbscan_frame(ri, tm, g, eps, mp), R.sklearn_labels(ri, tm, g, eps, mp)), (shape, eps, mp)


# ------------------------------------------------------------------------------------------------
# band pairs
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", C.SWEEP_EPS)
def test_band_pairs_sit_inside_the_band(eps):
    (ri, tm, g), f = C.band_pairs(eps)
    lo, hi = f["lo"], f["hi"]
    e2 = eps * eps
    assert float(lo) <= e2 * (1 - 2.0 ** -21) and float(np.nextafter(lo, np.float32(np.inf))) > e2 * (1 - 2.0 ** -21)
    assert float(hi) >= e2 * (1 + 2.0 ** -21) and float(np.nextafter(hi, np.float32(0))) < e2 * (1 + 2.0 ** -21)
    groups = f["groups"]
    assert len(groups) == 14
    inside = [gr for gr in groups if gr["in_band"]]
    assert any(gr["neighbour"] for gr in inside) and any(not gr["neighbour"] for gr in inside)
    for gr in groups:
        # no pair at exact equality but the one planted on purpose: the unmoved partner where eps is an fp32 number
        assert gr["planted"] == (gr["d2"] == e2) == (gr["step"] == 0 and f["exact_planted"])
        if gr["planted"]:
            assert not gr["neighbour"] and gr["d2f"] == np.float32(e2) and gr["in_band"]
        if gr["d2f"] < lo:                                     # the screen decides these, and decides them as fp64 does
            assert gr["neighbour"]
        if gr["d2f"] > hi:
            assert not gr["neighbour"]
    assert f["exact_planted"] == (eps in (1.5, 6.0, 40.0))
    if eps in (0.05, 0.45):   # a plain fp32 compare against float32(eps^2) decides one pair differently from the fp64 rule
        assert sum(1 for gr in groups if gr["in_band"] and gr["fp32_neighbour"] != gr["neighbour"]) >= 1
    # the groups are independent: no two points of different groups within 2 eps, none near the origin
    pts = np.array([gr["p"] for gr in f["groups"]] + [gr["q"] for gr in f["groups"]], np.float64)
    n = len(f["groups"])
    D = R.d2(pts[:, None], pts[None])
    same = (np.arange(2 * n)[:, None] % n) == (np.arange(2 * n)[None] % n)
    assert D[~same].min() > 4 * e2 and R.d2(pts, np.zeros(3)).min() > 4 * e2


@pytest.mark.parametrize("eps", C.SWEEP_EPS)
@pytest.mark.parametrize("mp", [2, 4, 10])
def test_band_expected_is_the_reference(eps, mp):
    (ri, tm, g), f = C.band_pairs(eps, mp)
    want = C.band_expected(f)
    assert np.array_equal(R.dbscan_frame(ri, tm, g, eps, mp), want)
    assert (want == 2).any() and want.max() >= 4
    tiles = C.tile_index(*C.BAND_SHAPE).reshape(-1)
    assert any(tiles[gr["pix"][0]] != tiles[gr["pix"][-1]] for gr in f["groups"] if gr["in_band"])


# ------------------------------------------------------------------------------------------------
# hand frames past the tile list
# ------------------------------------------------------------------------------------------------
def test_far_border():
    (ri, tm, g), f = C.far_border()
    assert f["T"] == 1030 and f["a_end_tile"] >= C.TILE_LIST and f["border_tile"] == f["b_tile"] == 0
    seg, cl, core = R.dbscan_frame(ri, tm, g, f["eps"], f["min_points"], with_clusters=True)
    assert np.array_equal(seg, f["want"])
    pix = np.nonzero(R.nonground(ri, tm, g).reshape(-1))[0]
    rank = {int(p): k for k, p in enumerate(pix)}
    b = rank[f["border"]]
    assert not core[b] and cl[b] == 0 and core[rank[f["a_end"]]]
    # its core neighbours: exactly the end of A (cluster 0, far tile) and one point of B (cluster 1, its own tile)
    P = R.points(ri, tm).reshape(-1, 3)[pix].astype(np.float64)
    nbr = np.nonzero((R.d2(P, P[b]) < f["eps"] ** 2) & core)[0]
    tile = C.tile_index(C.WIDE_H, C.WIDE_W).reshape(-1)
    assert sorted(cl[nbr].tolist()) == [0, 1] and sorted(tile[pix[nbr]].tolist()) == [0, f["a_end_tile"]]
    # without the far tile the border point would belong to cluster 1 (then numbered 0)
    ri2, tm2 = C.cut_high_tiles(ri, tm)
    assert R.dbscan_frame(ri2, tm2, g, f["eps"], f["min_points"]).reshape(-1)[f["border"]] == 3
    assert R.dbscan_frame(ri2, tm2, g, f["eps"], f["min_points"]).max() == 3


def test_origin_company():
    below = at = 0
    for Z, near, mp in C.ORIGIN_CASES:
        (ri, tm, g), f = C.origin_company(Z, near, mp)
        assert f["T"] == 1030 and (f["near_tiles"] >= C.TILE_LIST).all()
        assert (f["zero_tiles"] < C.TILE_LIST // 2).any() and (f["zero_tiles"] >= C.TILE_LIST).any()
        seg, cl, core = R.dbscan_frame(ri, tm, g, f["eps"], mp, with_clusters=True)
        assert np.array_equal(seg, f["want"]), (Z, near, mp)
        ng = R.nonground(ri, tm, g).reshape(-1)
        o0 = int(np.argmax(ri.reshape(-1)[ng] == 0))
        assert bool(core[o0]) == f["origin_core"] == (Z + near >= mp)
        below += Z + near == mp - 1
        at += Z + near == mp
    assert below >= 1 and at >= 1


# ------------------------------------------------------------------------------------------------
# kNN ties
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", C.KNN_SHAPES)
def test_knn_ties(H, W):
    p, f = C.knn_ties(H, W)
    a = E.compact(p)
    assert a.shape[0] == H * W
    tie = edge = 0
    for r in f["radii"]:
        t, e = C.knn_tie_facts(p, r)
        tie += t
        edge += e
        if r in (1.0, 2.0, 3.0) or r > 2.2:
            assert e > 0, r          # 1, 4, 9 and 5 are sums of two squares; so is 2
        if r == 2.0 or r == 3.0:
            assert t > 0, r
    assert tie > 0 and edge > 0
    # the claim's brute force agrees with the reference's kNN on a few interior queries
    q = np.array([(H // 2) * W + W // 2, 0, H * W - 1])
    nb = E.knn(a[q], a, 2.0)
    D = E.d2(a[q], a)
    for k in range(3):
        inr = np.nonzero(D[k] <= 4)[0]
        assert np.array_equal(nb[k, :min(12, inr.size)], inr[np.argsort(D[k, inr], kind="stable")][:12])
    assert (D[0] <= 4).sum() == 13 and np.sort(D[0])[11] == np.sort(D[0])[12] == 4


# ------------------------------------------------------------------------------------------------
# eval reference against cKDTree where no tie exists
# ------------------------------------------------------------------------------------------------
def test_eval_reference_against_ckdtree():
    spatial = pytest.importorskip("scipy.spatial")
    pairs = [C.folded_eval(2048, 160)[0], C.scattered_eval(8, 32769, 12000)[0]] + [c[1] for c in C.small_shapes()[2:]]
    rng = np.random.default_rng(1)
    for p1, p2 in pairs:
        s, q = E.compact(p2), E.compact(p1)
        q = q[np.sort(rng.choice(q.shape[0], min(1500, q.shape[0]), replace=False))]
        d, i = E.nn(q, s)
        tree = spatial.cKDTree(s.astype(np.float64))
        dk, ik = tree.query(q.astype(np.float64), k=min(2, s.shape[0]))
        dk, ik = dk.reshape(q.shape[0], -1), ik.reshape(q.shape[0], -1)
        assert np.allclose(np.sqrt(d.astype(np.float64)), dk[:, 0], rtol=1e-5, atol=1e-6)
        clear = dk[:, -1] > dk[:, 0] * (1 + 1e-4) + 1e-6 if dk.shape[1] > 1 else np.ones(q.shape[0], bool)   # no tie for first place
        assert clear.sum() > 0.9 * q.shape[0] and np.array_equal(i[clear], ik[clear, 0])
        # kNN: the twelve nearest within r, where the 12th and 13th are clearly apart and none sits at r
        r = 2.0
        nb = E.knn(q[:300], s, r)
        dd, ii = tree.query(q[:300].astype(np.float64), k=min(13, s.shape[0]), distance_upper_bound=r * (1 - 1e-6))
        compared = 0
        for k in range(min(300, q.shape[0])):
            fin = np.isfinite(dd[k][:12])
            got = nb[k][nb[k] >= 0]
            if np.all(np.diff(dd[k][np.isfinite(dd[k])]) > 1e-5):
                assert np.array_equal(got, ii[k][:12][fin]), k
                compared += 1
        assert compared > 0.9 * min(300, q.shape[0])
