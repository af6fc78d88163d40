"""The hostile values of tests/value_cases.py on the CPU: the oracle's quantiser follows the plainly stated conversion rule on all of Table A,
the table holds every class it is meant to, and scenes B and C reach -- in the oracle alone -- the values they are in the suite for.
tests/test_gpu_value_edges.py runs the same cases on the device."""
import numpy as np
import pytest

import launch_variants as lv
import value_cases as vc
from oracle import oracle as orc

F32 = np.float32


def _quotients(res, step):
    with np.errstate(all="ignore"):
        return (np.asarray(res, F32) / F32(step)).astype(F32)


def test_plain_statement_on_known_answers():
    """The statement the oracle is held to, on answers written out by hand."""
    res = np.array([0.5, -0.5, 1.5, 2.5, -2.5, 0.49999997, -0.50000006, 32767.5, 2147483520.0, 2.0 ** 31, -2.0 ** 31, -2147483904.0,
                    np.inf, -np.inf, np.nan, -0.0], F32)
    want = [1, -1, 2, 3, -3, 0, -1, 32768, 2147483520, vc.INT_MIN, vc.INT_MIN, vc.INT_MIN, vc.INT_MIN, vc.INT_MIN, vc.INT_MIN, 0]
    assert vc.plain_quantise(res, 1.0).tolist() == want
    assert vc.plain_quantise(np.array([0.0, 1.0], F32), 0.0).tolist() == [vc.INT_MIN, vc.INT_MIN]      # 0 / 0 and 1 / 0


def test_table_a_reaches_every_class():
    res, cls = vc.table_a()
    assert set(cls) == set(vc.CLASSES) and len(vc.CLASSES) == 6
    q = _quotients(res, vc.STEP_EXACT).astype(np.float64)
    by = lambda name: q[[c == name for c in cls]]
    # ties: k + 0.5 exactly, both signs, up to the last float32 that has a half
    t = by("ties")
    assert np.array_equal(np.abs(t) % 1.0, np.full(t.size, 0.5)) and {0.5, 32767.5, 65535.5, 2.0 ** 22 + 0.5, 2.0 ** 23 - 0.5} <= set(np.abs(t).tolist())
    assert (t > 0).sum() == (t < 0).sum() == 9
    # near ties: the floats next to 0.5 -- floor(x + 0.5) in float32 rounds 0.49999997 up to 1
    n = by("near ties")
    assert sorted(np.abs(n).tolist()) == [float(np.nextafter(F32(0.5), F32(0)))] * 2 + [float(np.nextafter(F32(0.5), F32(1)))] * 2
    assert np.floor(F32(0.49999997) + F32(0.5)) == 1.0 and vc.plain_quantise(F32(0.49999997), 1.0) == 0
    assert {32767.0, -32768.0, 32768.0, -32769.0, 65536.0, 75000.0} <= set(by("int16 wrap").tolist())
    e = by("int32 edge")
    assert {2147483520.0, 2.0 ** 31, -2.0 ** 31, -2147483904.0, 3e9, -3e9} <= set(e.tolist()) and (e > 1e19).any()
    assert np.isposinf(by("quotient overflows to inf")).all() and np.isposinf(_quotients(res[[c == "quotient overflows to inf" for c in cls]], vc.STEP_004)).all()
    r = res[[c == "non-finite residual" for c in cls]]
    assert sorted(r.view(np.uint32).tolist()) == sorted([0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0, 0x80000000, 1])
    # at step 0.04 the ties are no ties any more, the int32 edge stays one: both steps are needed
    assert not np.array_equal(vc.plain_quantise(res, vc.STEP_EXACT), vc.plain_quantise(res, vc.STEP_004))
    # the per-label steps: a zero step meets a zero and a non-zero residual; every step meets every residual through the image
    assert vc.LABEL_STEPS.tolist() == [F32(2.0 ** -5), F32(0.04), F32(1e-30), 0.0]
    for M in (20, 300):
        seg, rr, kp = vc.table_a_image(M)
        assert seg.min() == 0 and seg.max() == M + 1 and seg.size % 4 and seg.size > 1024
        lev = vc.label_levels(M + 2)
        assert set(lev[2:].tolist()) == {0, 1, 2, 3}
        for k in range(M + 2):
            assert np.array_equal(np.sort(rr[seg == k][: res.size].view(np.uint32)), np.sort(res.view(np.uint32))), (M, k)


@pytest.mark.parametrize("step", [float(s) for s in vc.UNIFORM_STEPS] + [float(s) for s in vc.LABEL_STEPS[2:]])
def test_oracle_uniform_quantiser_follows_the_plain_statement(step):
    res, cls = vc.table_a()
    got = orc.uniform_quantize(np.zeros(res.size, np.int32), res, step)
    want = vc.plain_quantise(res, step)
    assert got.dtype == np.int32 and np.array_equal(got, want), [(c, float(r), int(a), int(b)) for c, r, a, b in zip(cls, res, got, want) if a != b]
    if step == float(vc.STEP_EXACT):    # what the int16 container keeps of it
        q16 = dict(zip(_quotients(res, step).tolist(), got.astype(np.int16).tolist()))
        assert (q16[32767.0], q16[32768.0], q16[-32768.0], q16[-32769.0], q16[65536.0], q16[3e9], q16[2.0 ** 31]) == (32767, -32768, -32768, 32767, 0, 0, 0)


@pytest.mark.parametrize("M", [20, 300])
def test_oracle_quantisers_on_the_table_a_image(M):
    """The image form: label order, nnz, label 1 skipped; the non-uniform quantiser gives every label the level its key points were counted
    out for, and with it the per-label step (2^-5, 0.04, 1e-30, 0)."""
    seg, res, kp = vc.table_a_image(M)
    order = vc.label_order(seg)
    assert order.size == int((seg != 1).sum())
    for step in vc.UNIFORM_STEPS:
        assert np.array_equal(orc.uniform_quantize(seg, res, step), vc.plain_quantise(res[order], step)), (M, step)
    q, sal = orc.nonuniform_quantize(seg, res, kp, np.array(vc.LEVEL_KP_NUM), vc.LABEL_STEPS, vc.GROUND_LEVEL)
    assert np.array_equal(sal, vc.label_levels(M + 2))
    assert np.array_equal(q, vc.plain_quantise(res[order], vc.LABEL_STEPS[sal[seg[order]]]))


def test_scene_b_reaches_infinite_and_nan_predictions():
    b = vc.scene_b()
    tm, seg, ri = b["tm"], b["seg"], b["ri"]
    assert tm.shape == (31, 512, 3) and np.array_equal(tm[vc.B_ROW, :, 2].view(np.uint32), np.zeros(512, np.uint32)), "row 15 must have tz == +0.0 exactly"
    assert (tm[np.arange(31) != vc.B_ROW, :, 2] != 0).all()
    assert seg.min() == 0 and seg.max() == b["K"] - 1 and (seg == 1).any()
    for lab in range(b["K"]):       # each row owns pixels of row 15 and of an ordinary row, with returns on both
        assert (ri[vc.B_ROW][seg[vc.B_ROW] == lab] > 0).any() and (ri[3][seg[3] == lab] > 0).any(), lab
    pred = [orc.intra_predict(seg, b["model"][f], tm)[..., 0] for f in range(2)]
    on15 = np.zeros(seg.shape, bool)
    on15[vc.B_ROW] = True
    # ground (0, 0, -1, -1.7): 1.7 / +-0 on row 15, the sign that of the zero products; ground (0, 0, -1, 0): 0 / 0
    assert np.isposinf(pred[0][on15 & (seg == 0)]).any() and np.isneginf(pred[0][on15 & (seg == 0)]).any()
    assert np.isnan(pred[1][on15 & (seg == 0)]).all() and not np.isnan(pred[1][~on15]).any() and not np.isnan(pred[0]).any()
    assert np.isfinite(pred[0][~on15]).all()
    # the cancelling row: -d / +0 at its pixel in unfused arithmetic, a finite value with a contracted multiply-add
    a, bb, c, d = (F32(v) for v in b["model"][0, vc.L_CANCEL])
    w = b["cancel_col"]
    tx, ty = tm[vc.B_ROW, w, 0], tm[vc.B_ROW, w, 1]
    assert seg[vc.B_ROW, w] == vc.L_CANCEL and F32(a * tx) + F32(bb * ty) == 0 and float(a) * float(tx) + float(bb) * float(ty) != 0
    assert np.isneginf(pred[0][vc.B_ROW, w]) and np.isfinite(pred[0][vc.B_ROW, seg[vc.B_ROW] == vc.L_CANCEL]).sum() >= 7
    # (0, 0, 0, 3e38): the prediction itself, a residual whose quotient is -inf
    assert (pred[0][seg == vc.L_HUGE] == F32(3e38)).all()
    res = ri - pred[0]
    q = orc.uniform_quantize(seg, res, 0.04)
    order = vc.label_order(seg)
    quo = _quotients(res.reshape(-1)[order], 0.04)
    assert np.isneginf(quo).any() and np.isposinf(quo).any() and (q[~np.isfinite(quo)] == vc.INT_MIN).all()
    assert np.array_equal(q, vc.plain_quantise(res.reshape(-1)[order], 0.04))


def test_scene_b_has_a_pixel_that_is_a_point_only_in_the_reference_s_order():
    """(1e-8, 1, -1, 7): (a + b) + c is 0 in float32 -- the reference's order, the point branch, prediction d -- while a + (b + c) is 1e-8,
    the plane branch, another prediction."""
    b = vc.scene_b()
    a, bb, c, d = (F32(v) for v in vc.ROW_ORDER)
    assert F32(F32(a + bb) + c) == 0 and F32(a + F32(bb + c)) != 0
    pred = orc.intra_predict(b["seg"], b["model"][0], b["tm"])[..., 0]
    mine = b["seg"] == vc.L_ORDER
    assert (pred[mine] == d).all()
    tm = b["tm"][mine]
    with np.errstate(all="ignore"):
        other = -d / (a * tm[:, 0] + bb * tm[:, 1] + c * tm[:, 2])
    assert (other != d).all()


@pytest.mark.parametrize("form", sorted(vc.C_FORMS))
def test_scene_c_reaches_quotients_beyond_int32(form):
    """Every frame of the form: the far returns land on their pixels, stay out of the ground candidates (the seeded fit keeps its 800), the
    scene holds cluster_num distinct centres, far returns among them (every distance to them ties at temp's 1e10), squares stay finite, and at
    least one quantum has a float quotient >= 2^31 (x86: integer indefinite)."""
    H, W, B, M, count, growth = vc.C_FORMS[form]
    g = lv.geom_of(H, W)
    tm = orc.transform_map(g)
    assert (M <= 20 and lv.label_bytes(M) == 1) if form == "small" else M > 1022
    assert vc.C_R0 * growth ** (count - 1) < 1.8e19         # squares below 3.4e38
    for k in range(B):
        f, (hh, cc, r) = vc.scene_c_frame(form, k)
        ri = orc.project(f, g)
        assert np.allclose(ri[hh, cc], r, rtol=1e-6, atol=0)
        assert int((ri >= 1e5).sum()) == count and (tm[hh, cc, 2] > 0).all()
        assert orc.ground_candidates(ri, tm).shape[0] >= 800
        o = orc.compress_frame(f, g, tm, orc.ground_model(ri, tm, seed=7 + k), dict(orc.DEFAULT_CFG, cluster_num=M))
        assert len(set(o["fps_pix"].tolist())) == M and (ri.reshape(-1)[o["fps_pix"]] >= 1e5).sum() >= 2
        order = vc.label_order(o["seg_idx"])
        quo = _quotients(o["residual"].reshape(-1)[order], 0.04)
        assert np.isfinite(quo).all() and (quo >= 2.0 ** 31).any(), (form, k)
        assert (o["q"][np.abs(quo) >= 2.0 ** 31] == vc.INT_MIN).all() and np.array_equal(o["q"], vc.plain_quantise(o["residual"].reshape(-1)[order], 0.04))
