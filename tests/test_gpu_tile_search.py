"""The eval and DBSCAN searches on the MI355X (librpcc_eval.so, librpcc_seg.so) against the numpy references on the cases of
tests/tile_cases.py: more than one round of the tile list (T > 1024), more than one chunk of the row scan (H > 256), partial
row and column tiles, eps from 0.05 to 40, pairs inside the fp32 screen's band, BORDER's prune across tiles, the origin
point with company, and the kNN-12 where it ties.  tests/test_tile_cases.py asserts on the CPU that every case is what it
claims to be.  Every comparison is exact unless it says otherwise."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    import __graft_entry__ as ge
    ge.build()
    import dbscan_ref
    import eval_ref
    import tile_cases
    from rpcc_amd import dbscan, evaluate_metrics
    assert torch.cuda.is_available()
    return dict(torch=torch, R=dbscan_ref, E=eval_ref, C=tile_cases, db=dbscan, em=evaluate_metrics, dev=torch.device("cuda:0"))


# ------------------------------------------------------------------------------------------------
# DBSCAN
# ------------------------------------------------------------------------------------------------
def run(env, ri, tm, ground, eps, min_points, brute=False, stats=False):
    """numpy ri [B,H,W] (or [H,W]), tm [H,W,3], ground [B,4] (or [4]) -> numpy (seg, max_label[, stats])."""
    torch, dev = env["torch"], env["dev"]
    ri = np.asarray(ri, np.float32)
    ri = ri[None] if ri.ndim == 2 else ri
    ground = np.asarray(ground, np.float64).reshape(-1, 4)
    out = env["db"].dbscan_segment(torch.from_numpy(np.ascontiguousarray(ri)).to(dev), torch.from_numpy(np.ascontiguousarray(tm)).to(dev),
                                   torch.from_numpy(np.ascontiguousarray(ground)).to(dev), eps, min_points, brute_force=brute, stats=stats)
    return tuple(o.cpu().numpy() for o in out)


def check_dbscan(env, ri, tm, ground, eps, mp, want=None, tag=None):
    """seg and max_label == dbscan_ref.dbscan_frame, pruned and brute force; pruned == brute force bit for bit; a repeat run is
    identical.  -> (seg [H,W], pruned stats, brute-force stats)."""
    ref = env["R"].dbscan_frame(ri, tm, ground, eps, mp)
    if want is not None:
        assert np.array_equal(ref, want), tag
    seg, mx, st = run(env, ri, tm, ground, eps, mp, stats=True)
    bseg, bmx, bst = run(env, ri, tm, ground, eps, mp, brute=True, stats=True)
    bad = np.argwhere(seg[0] != ref)
    assert bad.shape[0] == 0, (tag, eps, mp, "pruned", bad.shape[0], bad[:4].tolist())
    bad = np.argwhere(bseg[0] != ref)
    assert bad.shape[0] == 0, (tag, eps, mp, "brute force", bad.shape[0], bad[:4].tolist())
    assert mx[0] == ref.max() == bmx[0], (tag, eps, mp)
    assert np.array_equal(seg, bseg)
    seg2, mx2 = run(env, ri, tm, ground, eps, mp)
    assert np.array_equal(seg, seg2) and np.array_equal(mx, mx2), (tag, eps, mp, "repeat")
    return seg[0], st[0], bst[0]


def check_batch(env, ri, tm, ground, eps, mp):
    """A batch of the frame and tile_cases.second_frame of it (one tm: the frames differ in ri) gives what each gives alone and
    what the reference gives."""
    C, R = env["C"], env["R"]
    ri2 = C.second_frame(ri, tm)
    ris, gs = np.stack([ri, ri2]), np.stack([ground, ground])
    seg, mx = run(env, ris, tm, gs, eps, mp)
    for b in range(2):
        s1, m1 = run(env, ris[b], tm, ground, eps, mp)
        assert np.array_equal(s1[0], seg[b]) and m1[0] == mx[b], b
        ref = R.dbscan_frame(ris[b], tm, ground, eps, mp)
        assert np.array_equal(seg[b], ref) and mx[b] == ref.max(), b
    assert not np.array_equal(seg[0], seg[1])
    bseg, bmx = run(env, ris, tm, gs, eps, mp, brute=True)
    assert np.array_equal(seg, bseg) and np.array_equal(mx, bmx)


@pytest.mark.parametrize("shape", [(2048, 160), (72, 4096)])
def test_dbscan_folded(env, shape):
    """T = 1280 with H > 256, and T = 1152: labels in tiles < 1024 depend on tiles >= 1024; pruning tests fewer pairs."""
    (ri, tm, g), f = env["C"].folded(*shape)
    assert f["T"] > 1024 and len(f["params"]) == 2
    for eps, mp in f["params"]:
        _, st, bst = check_dbscan(env, ri, tm, g, eps, mp, tag=shape)
        assert st[0] < bst[0], (shape, eps, mp, st, bst)


def test_dbscan_folded_batch(env):
    (ri, tm, g), f = env["C"].folded(2048, 160)
    check_batch(env, ri, tm, g, *f["params"][0])


@pytest.mark.parametrize("H,W,n", [(2048, 160, 20000), (8, 32768, 12000), (8, 32769, 12000)])
def test_dbscan_scattered(env, H, W, n):
    """Every tile's box spans the scene: every round keeps (nearly) every tile and the list fills to its capacity; T = 1280,
    T = 1024 exactly and T = 1025 with a last tile one column wide.  No stats threshold: the counter sums lane visits over the
    three modes and CORE stops early."""
    (ri, tm, g), f = env["C"].scattered(H, W, n)
    for eps, mp in f["params"]:
        seg, _, _ = check_dbscan(env, ri, tm, g, eps, mp, tag=(H, W))
    assert seg.max() >= 4 and (seg == 2).any()


def test_dbscan_scattered_batch(env):
    (ri, tm, g), f = env["C"].scattered(2048, 160, 20000)
    check_batch(env, ri, tm, g, *f["params"][0])


@pytest.mark.parametrize("k", range(6))
def test_dbscan_small_shapes(env, k):
    """(1, 1), (1, 1031), (7, 33), (9, 31), (257, 40), (300, 64): partial row tiles, partial column tiles, H > 256."""
    (ri, tm, g), _, f = env["C"].small_shapes()[k]
    assert (f["H"], f["W"]) == env["C"].SMALL_SHAPES[k]
    for eps, mp in f["params"]:
        check_dbscan(env, ri, tm, g, eps, mp, tag=(f["H"], f["W"]))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_dbscan_sweep(env, seed):
    """eps in {0.05, 0.45, 1.5, 6, 40} x min_points in {1, 2, 10, 50} on random blobs, 16 x 128 and 64 x 512: all noise, one
    cluster, thousands of clusters, the origin point core and not."""
    (ri, tm, g), f = env["C"].sweep_cloud(seed)
    for eps in f["eps"]:
        for mp in f["min_points"]:
            check_dbscan(env, ri, tm, g, eps, mp, tag=("sweep", seed))


@pytest.mark.parametrize("eps", [0.05, 0.45, 1.5, 6.0, 40.0])
def test_dbscan_band_pairs(env, eps):
    """Partners -3 ... +3 fp32 ulps around eps: pairs strictly inside the screen's band on both sides of the fp64 decision, and at
    eps 0.05 and 0.45 a pair that a plain fp32 compare against float32(eps^2) decides the other way."""
    C = env["C"]
    for mp in (2, 4, 10):
        (ri, tm, g), f = C.band_pairs(eps, mp)
        inside = [gr for gr in f["groups"] if gr["in_band"]]
        assert any(gr["neighbour"] for gr in inside) and any(not gr["neighbour"] for gr in inside)
        check_dbscan(env, ri, tm, g, eps, mp, want=C.band_expected(f), tag=("band", eps, mp))


def test_dbscan_far_border(env):
    """The border point's own tile holds a core point of cluster 1; cluster 0's only core point within eps lies in tile 1025."""
    (ri, tm, g), f = env["C"].far_border()
    seg, _, _ = check_dbscan(env, ri, tm, g, f["eps"], f["min_points"], want=f["want"], tag="far_border")
    assert seg.reshape(-1)[f["border"]] == 3


@pytest.mark.parametrize("Z,near,mp", [(6, 3, 10), (7, 3, 10), (3, 5, 8), (12, 2, 10)])
def test_dbscan_origin_company(env, Z, near, mp):
    """Zero-range pixels over both halves of the tile range and real points within eps of the origin in tiles >= 1024: one below
    the Z + near >= min_points flip, at it, and past it."""
    (ri, tm, g), f = env["C"].origin_company(Z, near, mp)
    assert f["origin_core"] == (Z + near >= mp)
    check_dbscan(env, ri, tm, g, f["eps"], mp, want=f["want"], tag=("origin", Z, near, mp))


# ------------------------------------------------------------------------------------------------
# eval
# ------------------------------------------------------------------------------------------------
EVERY_QUERY = 20000   # clouds up to this size are checked query by query, larger ones on a fixed sample
SAMPLE = 4096


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def img(env, a):
    return env["torch"].from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(env["dev"])[None]


def queries(q, seed=11):
    """The queries to check: all of a cloud of up to EVERY_QUERY points, else a fixed sample of SAMPLE; ordered along x so that
    the reference's chunks are compact and the device's answer, passed as `hint`, narrows its candidate set."""
    n = q.shape[0]
    qs = np.arange(n) if n <= EVERY_QUERY else np.random.default_rng(seed).choice(n, SAMPLE, replace=False)
    return qs[np.argsort(q[qs, 0], kind="stable")]


def check_nn(env, p1, p2):
    """Device NN of p1 / p2 (numpy f32 [H,W,3]) == eval_ref.nn in both directions, pruned == brute force.  -> nearest()'s tuple."""
    em, E, torch = env["em"], env["E"], env["torch"]
    t1, t2 = img(env, p1), img(env, p2)
    res = em.nearest(t1, t2, visits=True)
    bf = em.nearest(t1, t2, bruteforce=True)
    a, c = E.compact(p1), E.compact(p2)
    n = res[4].cpu().numpy()
    assert (n[0, 0], n[0, 1]) == (a.shape[0], c.shape[0])
    for (q, s, d, i, nq) in ((a, c, res[0], res[1], n[0, 0]), (c, a, res[2], res[3], n[0, 1])):
        dd, ii = d[0, :nq].cpu().numpy(), i[0, :nq].cpu().numpy()
        qs = queries(q)
        rd, ri = E.nn(q[qs], s, hint=ii[qs])
        bad = np.nonzero(ii[qs] != ri)[0]
        assert bad.size == 0, (bad.size, qs[bad[:4]].tolist(), ii[qs][bad[:4]].tolist(), ri[bad[:4]].tolist())
        assert np.array_equal(bits(dd[qs]), bits(rd))
    assert torch.equal(res[4], bf[4])
    for k, nq in ((0, n[0, 0]), (1, n[0, 0]), (2, n[0, 1]), (3, n[0, 1])):
        assert torch.equal(res[k][0, :nq], bf[k][0, :nq]), k
    return res


def check_normals(env, p, r, normal_sample=1500):
    """normals(..., neighbours=True) of numpy p [H,W,3] at radius r: the neighbour lists == eval_ref.knn (every query up to
    EVERY_QUERY points, else a sample), the normals by test_gpu_eval_metrics.test_normals' rule on a sample of those, pruned ==
    brute force including the lists."""
    em, E, torch = env["em"], env["E"], env["torch"]
    t = img(env, p)
    nrm, nbr = em.normals(t, r=r, neighbours=True)
    nrm_bf, nbr_bf = em.normals(t, r=r, bruteforce=True, neighbours=True)
    a = E.compact(p)
    n = a.shape[0]
    assert torch.equal(nbr[0, :n], nbr_bf[0, :n]) and torch.equal(nrm[0, :n], nrm_bf[0, :n]), r
    nb, nv = nbr[0, :n].cpu().numpy(), nrm[0, :n].cpu().numpy()
    qs = queries(a, seed=2)
    want = E.knn(a[qs], a, r, hint=nb[qs])
    bad = np.nonzero((want != nb[qs]).any(1))[0]
    assert bad.size == 0, (r, bad.size, qs[bad[:3]].tolist(), nb[qs][bad[:3]].tolist(), want[bad[:3]].tolist())
    if qs.size > normal_sample:
        qs = np.sort(np.random.default_rng(3).choice(qs, normal_sample, replace=False))
    for k in qs:
        cnt = int((nb[k] >= 0).sum())
        if cnt < 3:   # fewer than three neighbours within r: (0, 0, 1)
            assert np.array_equal(nv[k], [0.0, 0.0, 1.0]), (r, k)
            continue
        v, w, Cm = E.normal_of(a, nb[k])
        if np.dot(v, a[k].astype(np.float64)) > 0:
            v = -v
        if w[1] - w[0] > 1e-6 * w[2]:
            assert np.abs(nv[k] - v).max() <= 1e-9, (r, k)
        else:
            assert np.linalg.norm(Cm @ nv[k] - w[0] * nv[k]) <= 1e-9 * max(w[2], 1e-30) + 1e-12, (r, k)
        assert np.dot(nv[k], a[k].astype(np.float64)) <= 0, (r, k)
    return nb


@pytest.mark.parametrize("shape", [(2048, 160), (72, 4096)])
def test_nn_folded(env, shape):
    """The nearest cloud-2 point of a blanked point lies across tile 1024: found only by the second round of the list."""
    C = env["C"]
    (p1, p2), f = C.folded_eval(*shape)
    res = check_nn(env, p1, p2)
    i12 = res[1][0, :f["n1"]].cpu().numpy()
    assert C.nn_crossings(p1, p2, i12) >= 100
    vis = res[5][0].cpu().numpy()
    for c, nq in ((0, f["n1"]), (1, f["n2"])):
        assert vis[c, :nq].min() >= 1 and vis[c, :nq].max() <= f["T"]
        assert (vis[c, :nq] < f["T"]).any()   # pruning: some query visited fewer than T tiles


@pytest.mark.parametrize("H,W,n", [(2048, 160, 20000), (8, 32768, 12000), (8, 32769, 12000)])
def test_nn_scattered(env, H, W, n):
    """Every tile's box spans the scene and the clouds share no pixels: T = 1280, T = 1024 and T = 1025, whose one-column
    last tile holds the answer to the anchor query (every query checked)."""
    (p1, p2), f = env["C"].scattered_eval(H, W, n)
    assert f["T"] == {160: 1280, 32768: 1024, 32769: 1025}[W]
    check_nn(env, p1, p2)


@pytest.mark.parametrize("k", range(6))
def test_eval_small_shapes(env, k):
    _, (p1, p2), f = env["C"].small_shapes()[k]
    check_nn(env, p1, p2)
    for r in (0.5, 59.7):
        check_normals(env, p1, r)


@pytest.mark.parametrize("H,W", [(16, 96), (300, 64)])
def test_knn_ties(env, H, W):
    """The integer grid at r in {1, 2, 3, sqrt 2, sqrt 5}: ties for the 12th place (r = 2, 3), candidates at d == float32(r*r)
    (every r), tiles whose box bound equals the lane's bound."""
    C = env["C"]
    p, f = C.knn_ties(H, W)
    for r in f["radii"]:
        nb = check_normals(env, p, r)
        cnt = (nb >= 0).sum(1)
        want = {1.0: 5, 2.0: 12, 3.0: 12, 2.0 ** 0.5: 9, 5.0 ** 0.5: 12}[r]
        assert cnt.max() == want and (cnt == want).sum() > H * W // 2, r   # interior queries: the d <= float32(r*r) count


def test_normals_and_sums_folded(env):
    """kNN-12 at the default radius on the 2048 x 160 sheets (every query: 15 360 points), and the D1 / D2 sums of the eval
    variant against eval_ref.d1_d2 within test_d1_d2_against_numpy's 1e-9."""
    em, E, C = env["em"], env["E"], env["C"]
    (p1, p2), f = C.folded_eval(2048, 160)
    check_normals(env, p1, 59.7)
    check_normals(env, p1, 0.45)
    t1, t2 = img(env, p1), img(env, p2)
    res = em.nearest(t1, t2)
    nrm, _ = em.normals(t1)
    m = em.derive(em.frame_sums(t1, t2, res[1], res[3], nrm))
    pc1, pc2 = E.compact(p1), E.compact(p2)
    n1, n2 = pc1.shape[0], pc2.shape[0]
    want = E.d1_d2(pc1, pc2, res[1][0, :n1].cpu().numpy().astype(np.int64), res[3][0, :n2].cpu().numpy().astype(np.int64),
                   nrm[0, :n1].cpu().numpy())
    got = tuple(float(m[k][0]) for k in ("d1_mse_1", "d1_mse_2", "d2_mse_1", "d2_mse_2"))
    assert want[0] > 0 and want[2] > 0
    for g, w in zip(got, want):
        assert abs(g - w) <= 1e-9 * abs(w), (got, want)


def test_chamfer_flat_lists_past_the_tile_list(env):
    """[N,3] lists of 300 000 and 280 000 points through calc_chamfer_distance, the path a user takes: folded to rows of 2048
    they have T = 1216.  Indices and distance bits == eval_ref.nn on a 4096-query sample per direction; precision / recall are
    exact counts on the kernel's own distances."""
    em, E, C = env["em"], env["E"], env["C"]
    (a, b), f = C.flat_lists()
    assert f["T"] > 1024
    r = em.calc_chamfer_distance(a, b, out=False)
    info = r["chamfer_dist_info"]
    assert info["dist1"].shape[0] == a.shape[0] and info["dist2"].shape[0] == b.shape[0]
    for q, s, d, i in ((a, b, info["dist1"], info["idx1"]), (b, a, info["dist2"], info["idx2"])):
        qs = queries(q)
        assert qs.size == SAMPLE
        rd, ri = E.nn(q[qs], s, hint=i[qs])
        assert np.array_equal(i[qs], ri)
        assert np.array_equal(bits(d[qs]), bits(rd))
    t = np.float32(0.02 ** 2)
    assert r["precision"] == np.count_nonzero(info["dist1"] < t) / a.shape[0]
    assert r["recall"] == np.count_nonzero(info["dist2"] < t) / b.shape[0]
    assert 0 < r["recall"] < 1
