"""The C restatement (oracle/rpcc_oracle.c) against the reference's own C++ on seeded random inputs incl. edge cases, plus the
known-answer test of the restated glibc atan2f against this machine's libm.

The reference's side is stored: tests/golden/gen_golden_cpp.py ran the reference's C++ (compiled from its sources into oracle/_ref,
`make -C oracle ref`) on the inputs the _*_inputs() helpers below build, and kept SHA-256 digests of its outputs, and of the inputs
themselves, in tests/golden/ref_cpp_manifest.json.  The helpers are the one definition of those inputs, shared with the generator."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import feature_cases as fc
import value_cases as vc
from oracle import oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
MANIFEST = os.path.join(HERE, "golden", "ref_cpp_manifest.json")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def man():
    return json.load(open(MANIFEST))


def check_inputs(rec, **arrays):
    """The seeded inputs must be the ones the digests were made from (a NumPy generator change would show up here first)."""
    for k, v in arrays.items():
        assert sha(v) == rec["in"][k], "input %r is not the one the fixture was made from (numpy version?)" % k


def _atan2_inputs(rng, n):
    a = rng.uniform(-80, 80, n).astype(np.float32)
    b = rng.uniform(-80, 80, n).astype(np.float32)
    # elevation-like pairs, random bit patterns (inf/nan/denormals), axis cases
    z = rng.uniform(-30, 5, n).astype(np.float32)
    r = np.abs(rng.uniform(0.5, 80, n)).astype(np.float32)
    bits = rng.integers(0, 2**32, 2 * n, dtype=np.uint64).astype(np.uint32).view(np.float32)
    sp = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 3e38, 2**25, 2**-29], np.float32)
    sy, sx = np.meshgrid(sp, sp)
    y = np.concatenate([a, z, bits[:n], sy.ravel()])
    x = np.concatenate([b, r, bits[n:], sx.ravel()])
    return y, x


def test_atan2f_restatement_matches_libm():
    """KAT: fdlibm restatement == this container's glibc atan2f, bit for bit (NaNs compare as NaN)."""
    rng = np.random.default_rng(7)
    total = 0
    for _ in range(6):
        y, x = _atan2_inputs(rng, 1_000_000)
        o1 = np.empty_like(y)
        o2 = np.empty_like(y)
        orc.lib().orc_atan2f_array(orc._p(y), orc._p(x), orc._p(o1), C.c_long(y.size))
        orc.lib().orc_libm_atan2f_array(orc._p(y), orc._p(x), orc._p(o2), C.c_long(y.size))
        nan = np.isnan(o1) & np.isnan(o2)
        assert np.array_equal(o1.view(np.uint32)[~nan], o2.view(np.uint32)[~nan])
        total += y.size
    assert total >= 18_000_000


def _cloud(rng, n):
    xyz = rng.normal(0, 20, (n, 3)).astype(np.float32)
    xyz[:, 2] = rng.normal(-1, 1.5, n)
    xyz[: n // 50] = xyz[n // 50: 2 * (n // 50)] * np.float32(1.0000001)   # near-duplicates -> pixel collisions
    return xyz


def _project_inputs():
    rng = np.random.default_rng(11)
    xyz = _cloud(rng, 150_000)
    xyz[1000] = 0          # depth-0 point resets its pixel (cpp_modules.cpp:459) -- order dependent
    xyz[5] = [1e-30, 2e-30, 0]
    return xyz


@pytest.mark.parametrize("geom", sorted(orc.GEOMS))
def test_project_matches_reference_cpp(man, geom):
    rec = man["project"][geom]
    g = orc.LidarGeom(**orc.GEOMS[geom])
    xyz = _project_inputs()
    check_inputs(rec, xyz=xyz)
    got = orc.project(xyz, g)
    assert sha(got) == rec["ri"]


def _seg_and_ri(rng, h, w, nlab=102, empty_label=None):
    seg = rng.integers(0, nlab, (h, w)).astype(np.int32)
    # spatially coherent runs like real label maps
    seg = np.repeat(seg[:, ::8], 8, axis=1)[:, :w].copy()
    ri = rng.uniform(0.5, 80, (h, w)).astype(np.float32)
    ri[seg == 1] = 0
    if empty_label is not None:
        seg[seg == empty_label] = empty_label + 1
    return seg, ri


def _point_modeling_inputs():
    rng = np.random.default_rng(3)
    seg, ri = _seg_and_ri(rng, 64, 2000, empty_label=57)
    tm = orc.transform_map(orc.LidarGeom(**orc.GEOMS["Velodyne64E"]))
    return seg, ri, tm


def _model_param(pm):
    """The model rows intra_predict is fed: point_modeling's output plus hand-set rows."""
    mp = np.concatenate((np.zeros((pm.shape[0], 3)), pm[:, None].astype(np.float64)), -1)
    mp[0] = [0.0072, -0.054, -0.998, -1.76]
    mp[5] = [0.5, -0.5, 0.1, -3.0]
    mp[6] = [0.5, -0.5, 0.0, 7.0]                          # a+b+c == 0 -> constant prediction
    return mp


def test_point_modeling_and_predict_match(man):
    rec = man["point_modeling"]
    seg, ri, tm = _point_modeling_inputs()
    check_inputs(rec, seg=seg, ri=ri)
    pm_o = orc.point_modeling(ri, seg)
    assert sha(pm_o) == rec["pm"]
    assert pm_o.view(np.uint32)[57] == 0xFFC00000          # empty label -> NaN with this bit pattern
    mp = _model_param(pm_o)
    check_inputs(rec, mp=mp)
    pr_o = orc.intra_predict(seg, mp, tm)
    assert sha(pr_o) == rec["pred"]


QUANT_LEVELS = (np.array([30, 10, 3, 0]), np.array([0.04, 0.06, 0.08, 0.10]))


def _quantizer_inputs():
    rng = np.random.default_rng(4)
    seg, ri = _seg_and_ri(rng, 32, 2250)
    res = rng.normal(0, 1.0, seg.shape).astype(np.float32)
    res.reshape(-1)[:8] = [0.02, 0.06, -0.02, -0.06, 0.1, -0.1, 0.0, 1000.0]   # half-way cases
    kp = (rng.random(seg.shape) < 0.01).astype(np.int32) * rng.integers(1, 4, seg.shape).astype(np.int32)
    return seg, res, kp


def test_quantizers_match(man):
    rec = man["quantizers"]
    seg, res, kp = _quantizer_inputs()
    check_inputs(rec, seg=seg, res=res, kp=kp)
    q_o = orc.uniform_quantize(seg, res, 0.04)
    assert sha(q_o) == rec["q"]
    lk, la = QUANT_LEVELS
    qn_o, s_o = orc.nonuniform_quantize(seg, res, kp, lk, la, 2)
    assert sha(qn_o) == rec["qn"] and sha(s_o) == rec["sal"]


def _nan_canon(a):
    """NaNs with one bit pattern (the reference does not define theirs reproducibly: sign and payload are the compiler's and the chip's)."""
    a = np.array(a, np.float32)
    a[np.isnan(a)] = np.uint32(0x7FC00000).view(np.float32)
    return a


def _step_key(step):
    return "%.9g" % float(step)


def _value_table_inputs():
    """Table A of tests/value_cases.py as the 2-D arrays the reference's quantisers take."""
    seg, res, kp = vc.table_a_image(20)
    return seg.reshape(1, -1).copy(), res.reshape(1, -1).copy(), kp.reshape(1, -1).copy()


def test_quantizers_match_on_value_table(man):
    """Ties, near ties, the int16 wrap, the int32 edge, infinite and NaN quotients, zero steps: the restatement's stated conversion rule
    (INT_MIN for what C leaves undefined) is what the reference's x86 binary returns, for the uniform quantiser at both steps and for
    the non-uniform one with the per-label steps 2^-5, 0.04, 1e-30 and 0."""
    rec = man["value_table"]
    seg, res, kp = _value_table_inputs()
    check_inputs(rec, seg=seg, res=res, kp=kp)
    for step in vc.UNIFORM_STEPS:
        assert sha(orc.uniform_quantize(seg, res, float(step))) == rec["q"][_step_key(step)], step
    qn_o, s_o = orc.nonuniform_quantize(seg, res, kp, np.array(vc.LEVEL_KP_NUM), vc.LABEL_STEPS, vc.GROUND_LEVEL)
    assert sha(qn_o) == rec["qn"] and sha(s_o) == rec["sal"]
    assert (qn_o == vc.INT_MIN).any() and np.array_equal(s_o, vc.label_levels(22))


def _scene_b_inputs(frame):
    """Scene B of tests/value_cases.py: labels, the model rows of one frame, the transform map with tz == 0 on row 15, the range image, a key-point map that
    gives the labels all four salience levels."""
    b = vc.scene_b()
    return b["seg"], b["model"][frame], b["tm"], b["ri"], b["kp"]


@pytest.mark.parametrize("frame", [0, 1])
def test_predict_and_quantizers_match_on_scene_b(man, frame):
    """Predictions of +inf, -inf and NaN (compared with the NaNs' bits made equal), the (a + b) + c branch, the row that cancels only in
    unfused arithmetic, the prediction 3e38 -- and the quantisers on ri - pred."""
    rec = man["scene_b"][str(frame)]
    seg, mp, tm, ri, kp = _scene_b_inputs(frame)
    check_inputs(rec, seg=seg, mp=mp, tm=tm, ri=ri, kp=kp)
    pr_o = orc.intra_predict(seg, mp, tm)
    assert sha(_nan_canon(pr_o)) == rec["pred"]
    assert np.isinf(pr_o).any() and (frame == 0 or np.isnan(pr_o).any())
    with np.errstate(all="ignore"):
        res = ri - pr_o[..., 0]
    check_inputs(rec, res=_nan_canon(res))
    assert sha(orc.uniform_quantize(seg, res, 0.04)) == rec["q"]
    lk, la = QUANT_LEVELS
    qn_o, s_o = orc.nonuniform_quantize(seg, res, kp, lk, la, 2)
    assert sha(qn_o) == rec["qn"] and sha(s_o) == rec["sal"]


def _feature_inputs():
    rng = np.random.default_rng(5)
    seg, ri = _seg_and_ri(rng, 64, 2000)
    ri = (20 + 5 * np.sin(np.arange(2000) / 40.0)[None, :] + rng.normal(0, 0.05, (64, 2000))).astype(np.float32)
    ri[:, ::97] += 3.0                                                   # gaps -> occlusion gate
    ri[seg == 1] = 0
    return seg, ri


def test_features_match_on_written_cells(man):
    """The reference leaves feat/key_point_map uninitialised where it writes nothing
    (cpp_modules.cpp:38-43); compare on the cells the oracle writes and require the reference's
    written key points to be a superset-free match there."""
    rec = man["features"]
    seg, ri = _feature_inputs()
    check_inputs(rec, seg=seg, ri=ri)
    f_o, k_o = orc.extract_features_with_segment(ri, seg)
    wrote = f_o != 0
    assert sha(f_o[wrote]) == rec["f_written"]
    assert sha(k_o[k_o > 0]) == rec["k_written"]
    assert k_o.max() == 3 and (k_o == 1).any() and (k_o == 2).any()


FEATURE_PARAM_DRAWS = [(3, 8, 4, 8, 6)] + [tuple(int(v) for v in r) for r in np.stack([
    np.random.default_rng(77).integers(1, 6, 14), np.random.default_rng(78).integers(2, 13, 14),
    np.random.default_rng(79).integers(0, 7, 14), np.random.default_rng(80).integers(0, 13, 14),
    np.random.default_rng(81).integers(0, 11, 14)], 1)]


def _feature_sweep_inputs(params):
    fr, segments, sharp, less, flat = params
    rng = np.random.default_rng(1000 + 7 * fr + segments)
    h, w = 48, 1500
    seg = np.repeat(rng.integers(0, 30, (h, (w + 5) // 6)), 6, axis=1)[:, :w].astype(np.int32)
    ri = (20 + 5 * np.sin(np.arange(w) / 23.0)[None, :] + rng.normal(0, 0.04, (h, w))).astype(np.float32)
    ri[:, ::61] += 2.0
    ri[3, :] = 17.0                                                      # constant row: zero curvatures, ties
    seg[5, 40:] = 1                                                      # too few valid pixels
    ri[seg == 1] = 0
    return seg, ri


@pytest.mark.parametrize("params", FEATURE_PARAM_DRAWS)
def test_features_parameter_sweep_matches(man, params):
    """Key-point extraction with non-default feature_region / segments / sharp / less_sharp / flat counts (incl. zeros and
    less_sharp < sharp): the restatement against the reference's C++.  The reference leaves unwritten cells uninitialised
    (cpp_modules.cpp:38-43), so the generator ran it once in a fresh process with outputs large enough (288 KB) to be mmap'd
    zero pages: then the whole key point map can be compared, not only the cells the restatement writes."""
    rec = man["feature_sweep"][",".join(str(v) for v in params)]
    seg, ri = _feature_sweep_inputs(params)
    check_inputs(rec, seg=seg, ri=ri)
    f_o, k_o = orc.extract_features_with_segment(ri, seg, *params)
    wrote = f_o != 0
    assert sha(f_o[wrote]) == rec["f_written"], params
    assert sha(k_o) == rec["k"], params


def _feature_class_inputs(W, params):
    """The key-point image of a launch-variant case (tests/launch_variants.py), 96 rows high: outputs of at least 395 KB, which a fresh
    process gets as zero pages (see test_features_parameter_sweep_matches; at 197 KB it does not)."""
    return fc.feature_image(W, params, H=96)


@pytest.mark.parametrize("W,params", fc.FEATURE_PIN_DRAWS, ids=["%d-%s" % (w, "-".join(str(v) for v in p)) for w, p in fc.FEATURE_PIN_DRAWS])
def test_features_kernel_class_settings_match(man, W, params):
    """The settings at which tests/test_gpu_launch_variants.py holds the key-point kernels to the restatement -- more than 32 segments,
    flat_num 10, chunk lengths on both sides of 128, 256, 384 and 512, widths up to 4096 -- against the reference's C++, so that the
    restatement is not its own witness there."""
    rec = man["feature_classes"]["%d:%s" % (W, ",".join(str(v) for v in params))]
    seg, ri = _feature_class_inputs(W, params)
    check_inputs(rec, seg=seg, ri=ri)
    f_o, k_o = orc.extract_features_with_segment(ri, seg, *params)
    wrote = f_o != 0
    assert k_o.max() >= 1
    assert sha(f_o[wrote]) == rec["f_written"], (W, params)
    assert sha(k_o) == rec["k"], (W, params)


def _contour_inputs():
    rng = np.random.default_rng(6)
    seg, _ = _seg_and_ri(rng, 16, 1800)
    return seg


def test_contour_roundtrip_matches(man):
    rec = man["contour"]
    seg = _contour_inputs()
    check_inputs(rec, seg=seg)
    cm_o, sq_o = orc.extract_contour(seg)
    assert sha(cm_o) == rec["cm"] and sha(sq_o) == rec["sq"]
    assert sha(orc.recover_map(cm_o, sq_o)) == rec["recovered"]
    assert np.array_equal(orc.recover_map(cm_o, sq_o), seg)


def test_numpy_rows_match_c_rows():
    """a5/a7 written with the reference's NumPy expressions == the C rows (small case)."""
    g = orc.LidarGeom(H=16, W=200, vmax_deg=15, vmin_deg=-15)
    tm = orc.transform_map(g)
    rng = np.random.default_rng(8)
    ri = rng.uniform(1, 60, (16, 200)).astype(np.float32)
    ri[rng.random(ri.shape) < 0.2] = 0
    pc = orc.backproject(ri, tm)
    plane = np.array([0.01, -0.02, -0.999, -1.7])
    assert np.array_equal(orc.vertical_residual(pc, plane), orc.np_vertical_residual(pc, plane))
    cen = pc.reshape(-1, 3)[rng.choice(3200, 100, replace=False)]
    assert np.array_equal(orc.assign(ri, pc, tm, plane, cen), orc.np_assign(ri, pc, tm, plane, cen))


def test_np_mean_f32_restatement():
    rng = np.random.default_rng(9)
    for n in [1, 2, 7, 8, 9, 29, 127, 128, 129, 1000, 8191, 8192, 8193, 20000, 128000]:
        a = rng.uniform(0.5, 80, n).astype(np.float32)
        assert orc.np_mean_f32(a).view(np.uint32) == a.reshape(n, 1).mean().view(np.uint32), n
