"""-m gpu: the hostile values of tests/value_cases.py on the device, bit for bit against the CPU oracle.

Table A through the quantiser's own seam (ops.predict_quantize(..., residual=...)): ties, near ties, the int16 wrap, the int32 edge, quotients
that are infinite or NaN, zero steps -- int16 and int32 outputs, byte and uint16 labels, one step and per-label steps.  Scene B (a horizontal
beam: predictions of +inf, -inf and NaN) through every stage entry that sees a model row or a ground plane, and through both decoders.  Scene C
(returns at 1e6 m and beyond) through the fused batch entries.

Every value that is not NaN is compared by its bits and NaNs must sit at the same places; whether the NaN bit patterns are x86's as well is
printed, not asserted: the reference does not define them reproducibly."""
import numpy as np
import pytest

import launch_variants as lv
import value_cases as vc

pytestmark = pytest.mark.gpu
ACC = 0.02
DELTA = (0, 0.02, 0.04, 0.06)
LACC = np.array([2 * ACC] * 4) + np.array(DELTA)
SEED = 7


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    import rpcc_amd  # noqa: F401
    from rpcc_amd import _lib, ops
    from oracle import oracle as orc
    orc.lib()
    return dict(torch=torch, ops=ops, lib=_lib, orc=orc, dev=torch.device("cuda:0"))


def _to(env, a):
    return env["torch"].from_numpy(np.ascontiguousarray(a)).to(env["dev"])


def _np(t):
    return t.cpu().numpy()


def _same(got, exp, tag):
    """Shape and dtype; NaNs at the same places; every other value by its bits.  -> (NaNs compared, of them with the oracle's bit pattern)."""
    got, exp = np.ascontiguousarray(got), np.ascontiguousarray(exp)
    assert got.shape == exp.shape and got.dtype == exp.dtype, (tag, got.shape, exp.shape, got.dtype, exp.dtype)
    if got.dtype.kind != "f":
        bad = np.flatnonzero(got.reshape(-1) != exp.reshape(-1))
        assert bad.size == 0, (tag, bad.size, bad[:6], got.reshape(-1)[bad[:6]], exp.reshape(-1)[bad[:6]])
        return 0, 0
    g, e = got.reshape(-1), exp.reshape(-1)
    ng, ne = np.isnan(g), np.isnan(e)
    bad = np.flatnonzero(ng != ne)
    assert bad.size == 0, (tag, "NaN places", bad.size, bad[:6], g[bad[:6]], e[bad[:6]])
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    bad = np.flatnonzero((g.view(u) != e.view(u)) & ~ng)
    assert bad.size == 0, (tag, bad.size, bad[:6], g[bad[:6]], e[bad[:6]])
    return int(ng.sum()), int((g.view(u) == e.view(u))[ng].sum())


def _report_nans(what, counts):
    n, same = sum(c[0] for c in counts), sum(c[1] for c in counts)
    print("%s: %d NaN values compared by place, %d of them with the oracle's (x86's) bit pattern" % (what, n, same))


# ------------------------------------------------------------------------------------------------
# Table A
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_label", [False, True], ids=["one-step", "label-steps"])
@pytest.mark.parametrize("int16", [True, False], ids=["int16", "int32"])
@pytest.mark.parametrize("M", [20, 300])
def test_table_a_through_the_quantiser_seam(env, M, int16, per_label):
    """rpcc_predict_quantize / rpcc_predict_quantize_wide on a caller's residual: the integers, their order (labels ascending without label 1,
    row-major inside a label) and nnz equal the oracle's, which tests/test_value_cases.py holds to the plainly stated rule."""
    torch, ops, orc = env["torch"], env["ops"], env["orc"]
    seg, res, kp = vc.table_a_image(M)
    P, K = seg.size, M + 2
    d_seg = _to(env, seg.astype(np.uint16 if M > lv.MAX_CLUSTERS else np.uint8).reshape(1, P))
    assert d_seg.dtype == ops.label_dtype(M)
    d_res, d_ri = _to(env, res.reshape(1, P)), torch.zeros((1, P), dtype=torch.float32, device=env["dev"])
    d_tm, d_model = torch.zeros((P, 3), dtype=torch.float32, device=env["dev"]), torch.zeros((1, K, 4), dtype=torch.float32, device=env["dev"])
    runs = []
    if per_label:
        want, sal = orc.nonuniform_quantize(seg, res, kp, np.array(vc.LEVEL_KP_NUM), vc.LABEL_STEPS, vc.GROUND_LEVEL)
        runs.append((want, dict(acc=0.04, label_acc=_to(env, vc.LABEL_STEPS[sal].reshape(1, K)))))
    else:
        runs += [(orc.uniform_quantize(seg, res, float(step)), dict(acc=float(step))) for step in vc.UNIFORM_STEPS]
    for want, kw in runs:
        q, nnz, _ = ops.predict_quantize(d_ri, d_tm, d_seg, d_model, kw["acc"], M, int16=int16, label_acc=kw.get("label_acc"), residual=d_res)
        torch.cuda.synchronize()
        n = int(nnz[0])
        assert n == want.size == int((seg != 1).sum()), (M, int16, per_label, kw["acc"])
        got, want = _np(q)[0, :n], want.astype(np.int16 if int16 else np.int32)
        bad = np.flatnonzero(got != want)
        order = vc.label_order(seg)
        assert bad.size == 0, (M, int16, per_label, kw["acc"], bad.size,
                               sorted({(float(res[order[i]]), int(got[i]), int(want[i])) for i in bad}, key=lambda t: (t[0] != t[0], t[0]))[:12])
        assert not _np(q)[0, n:].any()


def test_table_a_residual_with_a_prediction_wanted(env):
    """The same seam with want_pred: the kernel form that predicts (from zero model rows) AND quantises the caller's residual."""
    torch, ops, orc = env["torch"], env["ops"], env["orc"]
    M = 20
    seg, res, _ = vc.table_a_image(M)
    P = seg.size
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device=env["dev"])
    q, nnz, pred = ops.predict_quantize(z(1, P), z(P, 3), _to(env, seg.astype(np.uint8).reshape(1, P)), z(1, M + 2, 4), 0.04, M, want_pred=True,
                                        residual=_to(env, res.reshape(1, P)))
    torch.cuda.synchronize()
    want = orc.uniform_quantize(seg, res, 0.04)
    assert int(nnz[0]) == want.size and np.array_equal(_np(q)[0, :want.size], want) and not _np(pred).any()


# ------------------------------------------------------------------------------------------------
# Scene B
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene_b(env):
    """Scene B on the device and the oracle's results on it, computed once: nothing writes into them."""
    orc = env["orc"]
    b = vc.scene_b()
    g, tm, ri, seg, K = b["g"], b["tm"], b["ri"], b["seg"], b["K"]
    assert np.array_equal(env["ops"].transform_map(g.H, g.W, g.horizontal_FOV, g.vertical_max, g.vertical_min), tm)
    model32 = b["model"].astype(np.float32)
    pred = np.stack([orc.intra_predict(seg, b["model"][f], tm)[..., 0] for f in range(2)])
    with np.errstate(all="ignore"):
        res = ri[None] - pred
    d = dict(b, model32=model32, pred=pred, res=res, P=g.H * g.W,
             d_ri=_to(env, np.stack([ri, ri])), d_tm=_to(env, tm), d_seg=_to(env, np.stack([seg, seg]).astype(np.uint8)), d_model=_to(env, model32),
             d_grounds=_to(env, b["grounds"]))
    return d


def test_scene_b_ground_mask_and_assignment(env, scene_b):
    """The ground planes (0, 0, -1, -1.7) and (0, 0, -1, 0) against the horizontal beam: the candidate mask of rpcc_ground_mask and the labels of
    rpcc_assign (the ground term of row 15 is infinite under the first plane, NaN under the second) equal the oracle's."""
    torch, ops, orc = env["torch"], env["ops"], env["orc"]
    s = scene_b
    g, tm, ri = s["g"], s["tm"], s["ri"]
    cfg = dict(orc.DEFAULT_CFG, cluster_num=vc.B_M)
    exp = [orc.segment(ri, tm, s["grounds"][f], cfg) for f in range(2)]
    temp, info = ops.ground_mask(s["d_ri"], s["d_tm"], s["d_grounds"], 0.1)
    seg = ops.assign(s["d_ri"], s["d_tm"], s["d_grounds"], _to(env, np.stack([o["centers"] for o in exp]).astype(np.float32)))
    torch.cuda.synchronize()
    for f, o in enumerate(exp):
        assert len(set(o["fps_pix"].tolist())) == vc.B_M
        assert np.array_equal((_np(temp)[f] > 0).reshape(g.H, g.W), o["mask"]) and int(info[f, 0]) == int(o["mask"].sum()), f
        _same(_np(seg)[f].astype(np.int64), o["seg_idx"], ("labels", f))
    row15 = exp[1]["seg_idx"][vc.B_ROW][ri[vc.B_ROW] > 0]
    assert row15.size and (row15 == 0).all(), "a NaN ground term wins the arg-nearest: every return of row 15 is ground under (0, 0, -1, 0)"


@pytest.mark.parametrize("wide", [False, True], ids=["u8", "u16"])
def test_scene_b_intra_predict(env, scene_b, wide):
    torch, ops = env["torch"], env["ops"]
    s = scene_b
    d_seg = _to(env, np.stack([s["seg"], s["seg"]]).astype(np.uint16)) if wide else s["d_seg"]
    pred = ops.intra_predict(d_seg, s["d_model"], s["d_tm"])
    torch.cuda.synchronize()
    _report_nans("intra_predict (%s)" % ("u16" if wide else "u8"), [_same(_np(pred)[f], s["pred"][f], ("pred", wide, f)) for f in range(2)])


@pytest.mark.parametrize("uniform", [True, False], ids=["uniform", "nonuniform"])
@pytest.mark.parametrize("int16", [True, False], ids=["int16", "int32"])
def test_scene_b_predict_quantize(env, scene_b, int16, uniform):
    """The ri - pred route with want_pred: predictions, integers, their order and nnz.  Non-uniform framework: the levels and per-label steps come
    from rpcc_salience on a key-point map that gives the labels all four levels."""
    torch, ops, orc = env["torch"], env["ops"], env["orc"]
    s = scene_b
    seg, K = s["seg"], s["K"]
    label_acc = None
    if not uniform:
        d_kp = _to(env, np.stack([s["kp"], s["kp"]]).astype(np.uint8))
        d_sal, label_acc = ops.salience(s["d_seg"], d_kp, vc.LEVEL_KP_NUM, LACC.astype(np.float32), vc.GROUND_LEVEL, vc.B_M)
    q, nnz, pred = ops.predict_quantize(s["d_ri"], s["d_tm"], s["d_seg"], s["d_model"], 2 * ACC, vc.B_M, want_pred=True, int16=int16, label_acc=label_acc)
    torch.cuda.synchronize()
    nans = []
    for f in range(2):
        nans.append(_same(_np(pred)[f].reshape(seg.shape), s["pred"][f], ("pred", f)))
        if uniform:
            want = orc.uniform_quantize(seg, s["res"][f], 2 * ACC)
        else:
            want, sal = orc.nonuniform_quantize(seg, s["res"][f], s["kp"], np.array(vc.LEVEL_KP_NUM), LACC.astype(np.float32), vc.GROUND_LEVEL)
            assert np.array_equal(_np(d_sal)[f], sal.astype(np.uint8)) and set(sal[2:].tolist()) == {0, 1, 2, 3}
        n = int(nnz[f])
        assert n == want.size, (f, n, want.size)
        got, want = _np(q)[f, :n], want.astype(np.int16 if int16 else np.int32)
        bad = np.flatnonzero(got != want)
        order = vc.label_order(seg)
        assert bad.size == 0, (int16, uniform, f, bad.size, [(float(s["res"][f].reshape(-1)[order[i]]), int(got[i]), int(want[i])) for i in bad[:8]])
    _report_nans("predict_quantize pred", nans)


def _scene_b_streams(env, s, uniform):
    """Per frame: a residual list that cycles through -32768, -1, 0, 1, 32767, the container's payload of it (oracle.pack_payload) and the
    oracle's decoder on that container."""
    orc = env["orc"]
    seg, K = s["seg"], s["K"]
    n = int((seg != 1).sum())
    sal = None if uniform else vc.label_levels(K).astype(np.uint8)
    out = []
    for f in range(2):
        q = vc.Q16_EDGES[(np.arange(n) + f) % vc.Q16_EDGES.size]
        assert set(q.tolist()) == {-32768, -1, 0, 1, 32767}
        od = orc.pack_payload(s["model32"][f], seg, sal, q)
        dec = orc.decode_frame(orc.bitstream_bytes(od, uniform=uniform), s["g"], s["tm"], accuracy=ACC, uniform=uniform, level_delta_acc=DELTA)
        assert np.array_equal(dec["seg_idx"], seg)
        out.append(dict(q=q, od=od, rec=np.ascontiguousarray(dec["ri_rec"][..., 0], np.float32), pc=np.ascontiguousarray(dec["pc_rec"], np.float32)))
    return n, sal, out


@pytest.mark.parametrize("uniform", [True, False], ids=["uniform", "nonuniform"])
def test_scene_b_decoders(env, scene_b, uniform):
    """rpcc_decode and rpcc_decompress_batch (the gated decode body) on scene B's rows and residuals at the ends of int16: the reconstructed range
    image and points -- infinite and NaN predictions, inf * 0 on the beam's z -- equal the oracle's decoder."""
    torch, ops = env["torch"], env["ops"]
    s = scene_b
    g, P, K = s["g"], s["P"], s["K"]
    n, sal, fr = _scene_b_streams(env, s, uniform)
    q16 = np.zeros((2, P), np.int16)
    for f in range(2):
        q16[f, :n] = fr[f]["q"]
    d_sal = None if uniform else _to(env, np.stack([sal, sal]))
    level_acc = 2 * ACC if uniform else list(LACC)
    rec, pc = ops.decode(s["d_seg"], _to(env, q16), s["d_model"], s["d_tm"], level_acc, salience=d_sal, want_points=True)
    # the same payloads as the entropy decoders leave them
    bits = np.stack([f_["od"]["contour_map"] for f_ in fr])
    seq = np.zeros((2, P), np.uint16)
    for f in range(2):
        seq[f, :fr[f]["od"]["idx_sequence"].size] = fr[f]["od"]["idx_sequence"]
    plen = np.array([[0 if uniform else K, bits.shape[1], 2 * f_["od"]["idx_sequence"].size, 16 * K, 2 * n] for f_ in fr], np.int64)
    st, seg2, rec2, pc2 = ops.decompress_batch(_to(env, bits), _to(env, seq), s["d_model"], _to(env, q16), _to(env, plen),
                                               torch.zeros((2, 5), dtype=torch.int32, device=env["dev"]), s["d_tm"], level_acc, g.H, g.W, salience=d_sal)
    torch.cuda.synchronize()
    assert _np(st).tolist() == [0, 0] and np.array_equal(_np(seg2).astype(np.int32), np.stack([s["seg"], s["seg"]]))
    nans = []
    for f in range(2):
        assert np.isinf(fr[f]["rec"]).any() and (np.isnan(fr[f]["pc"]).any() or f == 0)
        for name, got in (("decode rec", rec), ("decode pc", pc), ("batch rec", rec2), ("batch pc", pc2)):
            nans.append(_same(_np(got)[f], fr[f]["rec" if name.endswith("rec") else "pc"], (name, uniform, f)))
    _report_nans("decoders", nans)


# ------------------------------------------------------------------------------------------------
# Scene C
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", sorted(vc.C_FORMS))
def test_scene_c_through_the_fused_batch(env, form):
    """rpcc_compress_batch (small: byte labels, cluster_num 9) and rpcc_compress_batch_wide (wide: cluster_num 1100, the radix-sort kernels and
    the wide quantiser) on sweeps with returns at 1e6 m and beyond: range image, fitted ground plane, FPS pixels (ties at temp's 1e10), centres,
    labels, model rows (the sequential fp64 mean), integers (quotients beyond int32) and nnz equal the oracle's."""
    torch, ops, orc = env["torch"], env["ops"], env["orc"]
    H, W, B, M, _, _ = vc.C_FORMS[form]
    g = lv.geom_of(H, W)
    tm = orc.transform_map(g)
    geom = ops.make_geom(g.H, g.W, g.horizontal_FOV, g.vertical_max, g.vertical_min)
    frames = [vc.scene_c_frame(form, k)[0] for k in range(B)]
    offs = np.zeros(B + 1, np.int64)
    offs[1:] = np.cumsum([f.shape[0] for f in frames])
    buf = ops.BatchBuffers(B, geom, M, env["dev"], max_points=int(offs[-1]))
    assert buf.wide == (form == "wide")
    gms = torch.zeros((B, 4), dtype=torch.float64, device=env["dev"])
    ops.compress_batch(_to(env, np.concatenate(frames)), _to(env, offs), _to(env, tm), gms, buf, ground_seed=SEED, frame_ids=_to(env, np.arange(B, dtype=np.int64)))
    torch.cuda.synchronize()
    nans = []
    for k, f in enumerate(frames):
        ri = orc.project(f, g)
        gm = orc.ground_model(ri, tm, seed=SEED + k)
        o = orc.compress_frame(f, g, tm, gm, dict(orc.DEFAULT_CFG, cluster_num=M))
        mp = np.asarray(o["model_param"]).astype(np.float32)
        _same(_np(buf.ri)[k], ri, (form, k, "range image"))
        _same(_np(gms)[k], np.asarray(gm, np.float64), (form, k, "ground plane"))
        _same(_np(buf.cen_pix)[k], o["fps_pix"], (form, k, "FPS pixels"))
        _same(_np(buf.centers)[k], o["centers"].astype(np.float32), (form, k, "centres"))
        _same(_np(buf.seg)[k].astype(np.int64), o["seg_idx"], (form, k, "labels"))
        nans.append(_same(_np(buf.model)[k, :mp.shape[0]], mp, (form, k, "model rows")))
        n = int(buf.nnz[k])
        assert n == o["q"].shape[0], (form, k, n)
        _same(_np(buf.q16)[k, :n], o["q"].astype(np.int16), (form, k, "integers"))
    _report_nans("scene C model rows", nans)
