"""Reconstruction metrics on the MI355X (rpcc_amd.evaluate_metrics, librpcc_eval.so) against the numpy reference
(tests/eval_ref.py): nearest neighbours bit for bit, pruned = brute force, normals, D1 / D2, the batched entry and the
tools' --eval lines."""
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def env():
    import torch
    import __graft_entry__ as ge
    ge.build()
    import eval_ref
    from rpcc_amd import evaluate_metrics, ops, synth
    from oracle import oracle as orc
    assert torch.cuda.is_available()
    return dict(torch=torch, R=eval_ref, em=evaluate_metrics, ops=ops, synth=synth, GEOMS=orc.GEOMS, dev=torch.device("cuda:0"))


def _geom(env, name):
    gd = env["GEOMS"][name]
    args = (gd["H"], gd["W"], math.radians(gd["hfov_deg"]), math.radians(gd["vmax_deg"]), math.radians(gd["vmin_deg"]))
    return gd, env["ops"].make_geom(*args), env["torch"].from_numpy(env["ops"].transform_map(*args)).to(env["dev"])


def roundtrip(env, name, fids=None, acc=0.02, nonuniform=False, scene="default", frames=None):
    """Compress and decode a batch at `accuracy` acc -> (ri f32 [B,H,W], ri_rec, tm), all on the device."""
    torch, ops = env["torch"], env["ops"]
    gd, geom, tm = _geom(env, name)
    if frames is None:
        frames = [env["synth"].make_frame(f, gd["H"], gd["W"], vmax_deg=gd["vmax_deg"], vmin_deg=gd["vmin_deg"], scene=scene)
                  for f in fids]
    frames = [torch.as_tensor(np.asarray(f), dtype=torch.float32) for f in frames]
    B = len(frames)
    offs = torch.tensor([0] + list(np.cumsum([f.shape[0] for f in frames])), dtype=torch.int64, device=env["dev"])
    buf = ops.BatchBuffers(B, geom, 100, env["dev"], general=nonuniform)
    step = 2 * acc
    fid = torch.arange(B, dtype=torch.int64, device=env["dev"])
    ops.compress_batch(torch.cat(frames).to(env["dev"]), offs, tm, torch.zeros((B, 4), dtype=torch.float64, device=env["dev"]), buf,
                       ground_seed=1, frame_ids=fid, acc=step, nonuniform=ops.nonuniform_cfg(step) if nonuniform else None)
    if nonuniform:
        lacc = list(np.array([step] * 4) + np.array([0, 0.02, 0.04, 0.06]))
        rec, _ = ops.decode(buf.seg, buf.q16, buf.model, tm, lacc, salience=buf.salience)
    else:
        rec, _ = ops.decode(buf.seg, buf.q16, buf.model, tm, step)
    return buf.ri.clone(), rec, tm


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_nn(env, p1, p2, sample=None):
    """Device NN of p1 / p2 (f32 [B,H,W,3]) == numpy in both directions (every query, or a fixed sample), pruned == brute force."""
    em, R = env["em"], env["R"]
    res = em.nearest(p1, p2)
    bf = em.nearest(p1, p2, bruteforce=True)
    n = res[4].cpu().numpy()
    for b in range(p1.shape[0]):
        a, c = R.compact(p1[b].cpu().numpy()), R.compact(p2[b].cpu().numpy())
        assert (n[b, 0], n[b, 1]) == (a.shape[0], c.shape[0])
        for (q, s, d, i, nq) in ((a, c, res[0], res[1], n[b, 0]), (c, a, res[2], res[3], n[b, 1])):
            dd, ii = d[b, :nq].cpu().numpy(), i[b, :nq].cpu().numpy()
            qs = np.arange(nq) if sample is None else np.sort(np.random.default_rng(11).choice(nq, min(sample, nq), replace=False))
            rd, ri = R.nn(q[qs], s, hint=ii[qs])
            assert np.array_equal(bits(dd[qs]), bits(rd))
            assert np.array_equal(ii[qs], ri)
    assert env["torch"].equal(res[4], bf[4])
    for b in range(p1.shape[0]):
        for k, nq in ((0, n[b, 0]), (1, n[b, 0]), (2, n[b, 1]), (3, n[b, 1])):
            assert env["torch"].equal(res[k][b, :nq], bf[k][b, :nq])
    return res


def pts(env, ri, tm):
    return env["ops"].backproject(ri.contiguous(), tm)


@pytest.mark.parametrize("name", ["VelodyneVLP16", "Velodyne32E"])
@pytest.mark.parametrize("acc", [0.02, 0.1])
def test_nn_decoded_every_query(env, name, acc):
    ri, rec, tm = roundtrip(env, name, [300, 301], acc)
    p1, p2 = pts(env, ri, tm), pts(env, rec, tm)
    d1 = check_nn(env, p1, p2)[0]
    # physical bound, independent of the search: the same pixel of the other cloud is no farther than the depth error, up to
    # the fp32 rounding of the two points' coordinates (a few ulp of the range: 2^-20 of the farthest return)
    n = env["em"].nearest(p1, p2)[4].cpu().numpy()
    for b in range(2):
        err = float((rec[b] - ri[b]).abs().max())
        slack = float(ri[b].abs().max()) * 2.0 ** -20
        assert float(np.sqrt(d1[b, :n[b, 0]].cpu().numpy().astype(np.float64)).max()) <= err * (1 + 1e-6) + slack


@pytest.mark.parametrize("nonuniform", [False, True])
def test_nn_64x2048_and_example_sampled(env, nonuniform):
    ri, rec, tm = roundtrip(env, "Velodyne64E_2048", [310], 0.02, nonuniform=nonuniform)
    check_nn(env, pts(env, ri, tm), pts(env, rec, tm), sample=4096)
    z = np.load(os.path.join(HERE, "golden", "example_64E.npz"))
    ri, rec, tm = roundtrip(env, "Velodyne64E", acc=0.02, nonuniform=nonuniform, frames=[z["xyz"]])
    check_nn(env, pts(env, ri, tm), pts(env, rec, tm), sample=4096)


@pytest.mark.parametrize("scene", ["noise", "shell"])
def test_nn_adversarial_scenes(env, scene):
    ri, rec, tm = roundtrip(env, "VelodyneVLP16", [320], 0.1, scene=scene)
    check_nn(env, pts(env, ri, tm), pts(env, rec, tm))


def _img(env, a):
    return env["torch"].from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(env["dev"])[None]


def test_nn_adversarial_clouds(env):
    torch = env["torch"]
    rng = np.random.default_rng(3)
    H, W = 16, 96
    g = np.stack(np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32)), -1)
    base = np.concatenate([g + 1, np.full((H, W, 1), 2.0, np.float32)], -1)          # integer grid: exact distances
    cases = []
    ties = base.copy()
    ties[..., 0] += 0.5                                                               # every query between two targets
    cases.append((base, ties))
    dup = base.copy()
    dup[:, 1::2] = dup[:, 0::2]                                                       # duplicate points
    cases.append((base, dup))
    cases.append((base, base.copy()))                                                 # identical
    out = base.copy()
    out[3, 7] = (1000.0, 3.0, 2.0)                                                    # 1000 m outlier
    cases.append((base, out))
    blank = base.copy()
    blank[4:9] = 0                                                                    # rows blanked in one cloud
    cases.append((base, blank))
    one = np.zeros_like(base)
    one[10, 20] = (5.0, 5.0, 5.0)                                                     # a one-point cloud
    cases.append((base, one))
    zs = base.copy()
    zs[2, 2] = (1.0, -1.0, 0.0)                                                       # x + y + z == 0: not a point
    cases.append((zs, base))
    noisy = base + rng.normal(0, 0.3, base.shape).astype(np.float32)
    cases.append((noisy, base))
    for a, b in cases:
        check_nn(env, _img(env, a), _img(env, b))
    em = env["em"]
    p = _img(env, base)
    m = em.derive(em.frame_sums(p, p, *[em.nearest(p, p)[k] for k in (1, 3)], em.normals(p)[0]))
    assert float(m["cd_mean"][0]) == 0.0 and math.isinf(float(m["d1_psnr"][0])) and math.isinf(float(m["d2_psnr"][0]))
    assert int(R_count(env, zs)) == H * W - 1


def R_count(env, a):
    return env["R"].compact(a).shape[0]


def test_flat_lists_and_chamfer_dict(env):
    """A shuffled [N,3] list against another of different length through calc_chamfer_distance: indices and distances ==
    numpy; precision / recall are exact counts; cd*, mean, max, sum within 1e-12 of fp64 numpy on the kernel's values."""
    em, R = env["em"], env["R"]
    rng = np.random.default_rng(4)
    a = rng.uniform(-30, 30, (5000, 3)).astype(np.float32)
    b = (a[rng.permutation(5000)[:3700]] + rng.normal(0, 0.01, (3700, 3))).astype(np.float32)
    with pytest.raises(ValueError, match="points2"):
        em.calc_chamfer_distance(a, np.zeros((10, 3), np.float32), out=False)
    r = em.calc_chamfer_distance(a, b, out=False)
    info = r["chamfer_dist_info"]
    d1, i1 = R.nn(a, b)
    d2, i2 = R.nn(b, a)
    assert np.array_equal(bits(info["dist1"]), bits(d1)) and np.array_equal(info["idx1"], i1)
    assert np.array_equal(bits(info["dist2"]), bits(d2)) and np.array_equal(info["idx2"], i2)
    t = np.float32(0.02 ** 2)
    assert r["precision"] == np.count_nonzero(d1 < t) / 5000 and r["recall"] == np.count_nonzero(d2 < t) / 3700
    cd1 = np.sum(np.sqrt(d1).astype(np.float64)) / 5000
    cd2 = np.sum(np.sqrt(d2).astype(np.float64)) / 3700
    for key, want in (("cd1", cd1), ("cd2", cd2), ("mean", (cd1 + cd2) / 2), ("max", max(cd1, cd2)), ("sum", cd1 + cd2)):
        assert abs(r[key] - want) <= 1e-12 * abs(want), key
    p, q = r["precision"], r["recall"]
    assert r["f_score"] == (2 * p * q / (p + q) if p + q > 0 else 0.0)


def test_normals(env):
    torch, em, R = env["torch"], env["em"], env["R"]
    ri, rec, tm = roundtrip(env, "VelodyneVLP16", [330], 0.02)
    p = pts(env, ri, tm)
    nrm, nbr = em.normals(p, neighbours=True)
    nrm_bf, nbr_bf = em.normals(p, bruteforce=True, neighbours=True)
    n = int(em.nearest(p, p)[4][0, 0])
    assert torch.equal(nbr[0, :n], nbr_bf[0, :n]) and torch.equal(nrm[0, :n], nrm_bf[0, :n])
    a = R.compact(p[0].cpu().numpy())
    nb, nv = nbr[0, :n].cpu().numpy(), nrm[0, :n].cpu().numpy()
    qs = np.sort(np.random.default_rng(2).choice(n, 3000, replace=False))
    assert np.array_equal(R.knn(a[qs], a, 59.7, hint=nb[qs]), nb[qs])
    for k in qs:
        v, w, C = R.normal_of(a, nb[k])
        if np.dot(v, a[k].astype(np.float64)) > 0:
            v = -v
        if w[1] - w[0] > 1e-6 * w[2]:
            assert np.abs(nv[k] - v).max() <= 1e-9, k
        else:
            assert np.linalg.norm(C @ nv[k] - w[0] * nv[k]) <= 1e-9 * max(w[2], 1e-30) + 1e-12
        if (nb[k] >= 0).sum() >= 3:
            assert np.dot(nv[k], a[k].astype(np.float64)) <= 0
    # fewer than three neighbours within r: (0, 0, 1)
    sparse = np.zeros((8, 32, 3), np.float32)
    sparse[0, :10] = np.stack([np.arange(10) * 5.0 + 3, np.ones(10), np.ones(10)], -1)
    sparse[1, 0] = (3.5, 1.0, 1.0)
    ns, nbs = em.normals(_img(env, sparse), r=1.0, neighbours=True)
    cnt = (nbs[0, :11] >= 0).sum(1).cpu().numpy()
    assert cnt.max() < 3 and np.array_equal(ns[0, :11].cpu().numpy(), np.tile([0.0, 0.0, 1.0], (11, 1)))


def test_d1_d2_against_numpy(env):
    em, R = env["em"], env["R"]
    ri, rec, tm = roundtrip(env, "VelodyneVLP16", [340], 0.1)
    p1, p2 = pts(env, ri, tm), pts(env, rec, tm)
    a, c = p1[0].cpu().numpy(), p2[0].cpu().numpy()
    cd = em.calc_chamfer_distance(a, c, out=False)["chamfer_dist_info"]
    nrm, _ = em.normals(p1)
    pc1, pc2 = R.compact(a), R.compact(c)
    n1 = nrm[0, :pc1.shape[0]].cpu().numpy()
    want = R.d1_d2(pc1, pc2, cd["idx1"].astype(np.int64), cd["idx2"].astype(np.int64), n1)
    for given in (False, True):   # the PSNR function's convention: idx1 = cloud 2 -> cloud 1 (the Chamfer dict's idx2)
        kw = dict(idx1=cd["idx2"], idx2=cd["idx1"]) if given else {}
        pp, pl = em.calc_point_to_point_plane_psnr(a, c, out=False, **kw)
        got = (pp["mse_1"], pp["mse_2"], pl["mse_1"], pl["mse_2"])
        for g, w in zip(got, want):
            assert abs(g - w) <= 1e-9 * abs(w), (given, got, want)
        assert pp["psnr_1"] == pytest.approx(10 * np.log10(3 * 59.7 ** 2 / want[0]), rel=1e-12)
    with pytest.raises(ValueError):
        em.calc_point_to_point_plane_psnr(a, c, idx1=cd["idx2"][:-1], idx2=cd["idx1"], out=False)


def test_quality_batch_equals_single_frames_and_repeats(env):
    torch, em = env["torch"], env["em"]
    scenes = ["default", "noise", "shell", "corridor"]
    gd = env["GEOMS"]["VelodyneVLP16"]
    frames = [env["synth"].make_frame(400 + i, gd["H"], gd["W"], vmax_deg=gd["vmax_deg"], vmin_deg=gd["vmin_deg"],
                                      scene=scenes[i % 4]) for i in range(64)]
    ri, rec, tm = roundtrip(env, "VelodyneVLP16", acc=0.05, frames=frames)
    rec[5] = 0                                             # an empty reconstruction: NaN for that frame, nothing else changes
    m1 = em.quality_batch(ri, rec, tm)
    m2 = em.quality_batch(ri, rec, tm)
    keys = ["cd1", "cd2", "cd_mean", "f_score", "precision", "recall", "d1_mse_1", "d1_mse_2", "d1_psnr", "d2_mse_1", "d2_mse_2", "d2_psnr"]
    for k in keys:
        assert m1[k].shape == (64,) and m1[k].dtype == torch.float64
        assert torch.equal(m1[k].isnan(), m2[k].isnan()) and torch.equal(m1[k].nan_to_num(), m2[k].nan_to_num()), k
        assert bool(m1[k][5].isnan()) and not bool(m1[k][torch.arange(64) != 5].isnan().any()), k
    for b in range(64):
        s = em.quality_batch(ri[b:b + 1], rec[b:b + 1], tm)
        for k in keys:
            assert torch.equal(s[k].nan_to_num(), m1[k][b:b + 1].nan_to_num()), (b, k)
    p1, p2 = pts(env, ri[:1], tm)[0].cpu().numpy(), pts(env, rec[:1], tm)[0].cpu().numpy()
    c = em.calc_chamfer_distance(p1, p2, out=False)
    pp, pl = em.calc_point_to_point_plane_psnr(p1, p2, out=False)
    assert (c["mean"], c["f_score"], pp["psnr_mean"], pl["psnr_mean"]) == \
        tuple(float(m1[k][0]) for k in ("cd_mean", "f_score", "d1_psnr", "d2_psnr"))


def _metric_lines(text):
    out = {}
    for label in ("Chamfer Distance (mean)", "F1 score (threshold=0.02)", "Point-to-Point PSNR (r=59.7)", "Point-to-Plane PSNR (r=59.7)"):
        lines = [ln for ln in text.splitlines() if ln.startswith("    %s: " % label)]
        assert len(lines) == 1, label
        out[label] = float(lines[0].split(": ", 1)[1])
    return out


def test_cli_eval_lines(env, tmp_path, capsys):
    em = env["em"]
    from rpcc_amd.dataset import build_dataset
    from rpcc_amd.tools import compress as tc, decompress as td
    z = np.load(os.path.join(HERE, "golden", "example_64E.npz"))
    src = tmp_path / "frame.bin"
    np.concatenate((z["xyz"], np.zeros((z["xyz"].shape[0], 1), np.float32)), 1).astype(np.float32).tofile(src)
    out, rec = tmp_path / "frame.rpcc", tmp_path / "rec.bin"
    common = ["--lidar", "Velodyne64E"]
    capsys.readouterr()
    tc.compress(tc.make_parser().parse_args(["--input", str(src), "--output", str(out), "--eval"] + common))
    printed_c = _metric_lines(capsys.readouterr().out)
    td.decompress(tc.make_parser().parse_args(["--input", str(out), "--output", str(rec), "--eval", "--original_point_cloud", str(src)]
                                              + common))
    printed_d = _metric_lines(capsys.readouterr().out)
    assert printed_c == printed_d
    orig = build_dataset(lidar_type="Velodyne64E").load_range_image_points_from_file(str(src))[0]
    recp = np.fromfile(rec, dtype=np.float32).reshape(-1, 4)[:, :3]
    c = em.calc_chamfer_distance(orig, recp, out=False)
    pp, pl = em.calc_point_to_point_plane_psnr(orig, recp, out=False)
    assert printed_c == {"Chamfer Distance (mean)": c["mean"], "F1 score (threshold=0.02)": c["f_score"],
                         "Point-to-Point PSNR (r=59.7)": pp["psnr_mean"], "Point-to-Plane PSNR (r=59.7)": pl["psnr_mean"]}
    with pytest.raises(ValueError, match="original_point_cloud"):
        td.decompress(tc.make_parser().parse_args(["--input", str(out), "--output", str(rec), "--eval"] + common))
