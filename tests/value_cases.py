"""Hostile VALUES for the quantiser, the predictor and the decoder (numpy and the CPU oracle only; tests/test_value_cases.py asserts on the
CPU that the cases reach what they are here for, tests/test_gpu_value_edges.py runs them on the device, tests/test_oracle_vs_ref.py pins the
oracle on them against the reference's C++).

The rest of the suite feeds the kernels what a clean sweep produces: ranges below 120 m, quotients residual / step below 75 000.  Here only
the values are hostile -- every label stays within 0 .. M + 1, every salience level within the configured ones, every size is a legal one, and
nothing is indexed by a hostile value.

Table A  residuals whose quotient sits on a rounding tie, next to one, at the int16 wrap, at the int32 edge, beyond it, or is not finite.
Scene B  a lidar with a horizontal beam (tz == 0.0 on row 15) and injected model rows whose prediction there is +inf, -inf or NaN, whose
         a + b + c is zero only in the reference's order of additions, or whose a * tx + b * ty cancels only without contraction.
Scene C  far returns (1e6 m and beyond) in a sweep: every FPS distance to them ties at the 1e10 cap of temp, the clusters that hold them have
         residuals whose quotient leaves int32."""
import functools

import numpy as np

import launch_variants as lv

INT_MIN = -2 ** 31
F32 = np.float32

# ------------------------------------------------------------------------------------------------
# Table A
# ------------------------------------------------------------------------------------------------
STEP_EXACT, STEP_004 = F32(2.0 ** -5), F32(0.04)      # residual = float32(quotient * 2^-5): the quotient is exact at the first step
UNIFORM_STEPS = (STEP_EXACT, STEP_004)
LABEL_STEPS = np.array([2.0 ** -5, 0.04, 1e-30, 0.0], F32)      # per-label steps (label_acc): level l of LEVEL_KP_NUM has step LABEL_STEPS[l]
LEVEL_KP_NUM = (30, 10, 3, 0)
GROUND_LEVEL = 2


def _both(vals):
    return [s * float(v) for v in vals for s in (1.0, -1.0)]


QUOTIENTS = {
    "ties": _both([k + 0.5 for k in (0, 1, 2, 7, 32766, 32767, 65535, 2 ** 22, 2 ** 23 - 1)]),
    "near ties": _both([np.nextafter(F32(0.5), F32(0)), np.nextafter(F32(0.5), F32(1))]),        # 0.49999997, 0.50000006
    "int16 wrap": _both([32767, 32768, 32769, 65536]) + [75000.0],
    # 2147483520: the largest float below 2^31 (valid); 2^31: indefinite; -2^31: valid, equals INT_MIN; the next float below: indefinite
    "int32 edge": [2147483520.0, 2.0 ** 31, -2.0 ** 31, float(np.nextafter(F32(-2.0 ** 31), F32(-np.inf))), 3e9, -3e9, 1e20],
}
# residuals given as they are (bit patterns for the NaNs: either sign)
RESIDUALS = {
    "quotient overflows to inf": np.array([3e38], F32),
    "non-finite residual": np.array([0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x00000000, 0x80000000, 0x00000001], np.uint32).view(F32),
}
CLASSES = tuple(QUOTIENTS) + tuple(RESIDUALS)


@functools.lru_cache(maxsize=None)
def table_a():
    """-> (residuals f32 [n], class name per residual)."""
    res, cls = [], []
    for name, qs in QUOTIENTS.items():
        res.append((np.asarray(qs, np.float64) * 2.0 ** -5).astype(F32))
        cls += [name] * len(qs)
    for name, r in RESIDUALS.items():
        res.append(r)
        cls += [name] * r.size
    res = np.concatenate(res)
    res.setflags(write=False)
    return res, tuple(cls)


def plain_quantise(res, step):
    """The rule, stated plainly: float32 division; rounding half away from zero, done in float64 on the float32 quotient (exact: a float32
    plus 0.5 is a float64); INT_MIN -- x86's "integer indefinite" -- unless the rounded value is finite and lies in [-2^31, 2^31)."""
    with np.errstate(all="ignore"):
        q = (np.asarray(res, F32) / np.asarray(step, F32)).astype(F32)
        r = np.copysign(np.floor(np.abs(q.astype(np.float64)) + 0.5), q.astype(np.float64))
    ok = np.isfinite(r) & (r >= -2.0 ** 31) & (r < 2.0 ** 31)
    return np.where(ok, r, float(INT_MIN)).astype(np.int64).astype(np.int32)


def label_levels(K):
    """Salience level of every label of the Table A image: label 0 the ground level, label 1 the last one, label k >= 2 level k % 4 (its
    key points are counted out so: table_a_image)."""
    lv_ = np.arange(K) % 4
    lv_[0], lv_[1] = GROUND_LEVEL, len(LEVEL_KP_NUM) - 1
    return lv_.astype(np.int32)


def level_keypoints(seg, K):
    """A key-point map (int32, seg's shape) that gives label k >= 2 exactly LEVEL_KP_NUM[k % 4] key points, on its first pixels in row-major
    order: with LEVEL_KP_NUM as level_kp_num a label of 30 pixels or more then takes salience level k % 4."""
    kp = np.zeros(seg.size, np.int32)
    flat = np.asarray(seg).reshape(-1)
    for k in range(2, K):
        kp[np.flatnonzero(flat == k)[: LEVEL_KP_NUM[k % 4]]] = 1 + k % 3
    return kp.reshape(np.shape(seg))


@functools.lru_cache(maxsize=4)
def table_a_image(M):
    """The Table A residuals as one image of P = n * (M + 2) * repeats + 3 pixels (at least 2500 and no multiple of four: several tiles of
    the quantiser, a last quad that is cut short): pixel p holds
    residual p % n and label (p // n) % (M + 2), so every residual meets every label -- label 1, which is skipped, among them -- and, through
    label_levels, every per-label step.  -> (seg int32 [P], residual f32 [P], key points int32 [P]): label k >= 2 carries LEVEL_KP_NUM[k % 4]
    key points, which is what gives it level k % 4 in the non-uniform quantiser."""
    res, _ = table_a()
    n, K = res.size, M + 2
    assert n >= 30, "a label of fewer than 30 pixels takes the last level whatever its key points"
    P = n * K * -(-2500 // (n * K)) + 3
    p = np.arange(P)
    seg = ((p // n) % K).astype(np.int32)
    out = (seg, res[p % n].copy(), level_keypoints(seg, K))
    for a in out:
        a.setflags(write=False)
    return out


def label_order(seg):
    """Pixels in the order of the quantised list: labels ascending without label 1, row-major inside a label."""
    seg = np.asarray(seg).reshape(-1)
    order = np.argsort(seg, kind="stable")
    return order[seg[order] != 1]


# ------------------------------------------------------------------------------------------------
# Scene B: the horizontal beam
# ------------------------------------------------------------------------------------------------
B_H, B_W, B_VMAX, B_VMIN, B_ROW, B_M = 31, 512, 15.0, -15.0, 15, 20
B_BLOCK = 8                 # labels change every 8 columns, the same in every row: each label owns pixels of row 15 and of ordinary rows
B_GROUNDS = np.array([[0.0, 0.0, -1.0, -1.7], [0.0, 0.0, -1.0, 0.0]])      # frame 0 / frame 1: the second gives the 0 / 0 prediction on row 15
L_ORDER, L_CANCEL, L_HUGE, L_PLANE, L_POINT = 2, 3, 4, 5, 6
ROW_ORDER = (1e-8, 1.0, -1.0, 7.0)      # (a + b) + c == 0 in fp32, a + (b + c) is not
ROW_HUGE = (0.0, 0.0, 0.0, 3e38)
CANCEL_C, CANCEL_D = -1.0, 2.5


def b_geom():
    from oracle import oracle as orc
    return orc.LidarGeom(B_H, B_W, 360.0, B_VMAX, B_VMIN)


def b_labels(K=B_M + 2):
    """int32 [H,W]: label ((w // 8) % K) in every row."""
    return np.broadcast_to(((np.arange(B_W) // B_BLOCK) % K).astype(np.int32), (B_H, B_W)).copy()


def find_cancel_row(tm, seg):
    """A row (a, b, c, d) and a pixel (row 15, column w) of label L_CANCEL with fl(a * tx) + fl(b * ty) == 0 while a * tx + b * ty is not
    zero exactly: the denominator of the prediction is +-0 in unfused arithmetic (the reference's, -ffp-contract=off here) and a small
    non-zero number under a contracted multiply-add.  Deterministic search over the label's columns."""
    rng = np.random.default_rng(15)
    cols = np.flatnonzero(seg[B_ROW] == L_CANCEL)
    for _ in range(4000):
        w = int(rng.choice(cols))
        tx, ty = tm[B_ROW, w, 0], tm[B_ROW, w, 1]
        if tx == 0 or ty == 0:
            continue
        a = F32(rng.uniform(0.5, 2.0))
        b = F32(-(F32(a * tx)) / ty)
        if F32(a * tx) + F32(b * ty) == 0 and float(a) * float(tx) + float(b) * float(ty) != 0.0 and F32(F32(a + b) + F32(CANCEL_C)) != 0:
            return (float(a), float(b), CANCEL_C, CANCEL_D), w
    raise AssertionError("no cancelling row found")


@functools.lru_cache(maxsize=None)
def scene_b():
    """dict(g, tm, ri f32 [H,W] (a synthetic sweep), grounds f64 [2,4], seg int32 [H,W], model f64 [2,K,4], cancel_col, kp int32 [H,W]): two frames that
    differ in the ground row only."""
    from oracle import oracle as orc
    with lv._IMPORT_LOCK:
        from rpcc_amd import synth
    g = b_geom()
    tm = orc.transform_map(g)
    ri = orc.project(synth.make_frame(1500, B_H, B_W, vmax_deg=B_VMAX, vmin_deg=B_VMIN).numpy(), g)
    K = B_M + 2
    seg = b_labels(K)
    cancel, col = find_cancel_row(tm, seg)
    model = np.zeros((2, K, 4))
    model[:, :, 3] = 5.0 + 1.5 * np.arange(K)[None, :]                  # point rows
    model[:, 1] = 0.0
    model[:, L_ORDER], model[:, L_CANCEL], model[:, L_HUGE] = ROW_ORDER, cancel, ROW_HUGE
    model[:, L_PLANE] = (0.3, -0.2, 0.9, -6.0)                          # an ordinary plane
    model[:, 0] = B_GROUNDS
    return dict(g=g, tm=tm, ri=ri, grounds=B_GROUNDS.copy(), seg=seg, model=model, cancel_col=col, K=K, kp=level_keypoints(seg, K))


Q16_EDGES = np.array([-32768, -1, 0, 1, 32767], np.int16)


# ------------------------------------------------------------------------------------------------
# Scene C: far returns
# ------------------------------------------------------------------------------------------------
# form -> (H, W, frames, cluster_num, far returns per frame, growth of their ranges)
C_FORMS = {"small": (7, 301, 3, 9, 40, 1.7), "wide": (16, 1800, 2, 1100, 1300, 1.02)}
C_R0 = 1e6


def c_rows(H):
    """The image rows above the horizon (the far returns must not become ground candidates: z > 0)."""
    el = lv.VMIN_DEG + (lv.VMAX_DEG - lv.VMIN_DEG) * np.arange(H) / (H - 1)
    return [int(h) for h in np.flatnonzero(el > 0.5)]


@functools.lru_cache(maxsize=8)
def scene_c_frame(form, k):
    """Scene k of launch_variants' builder (it keeps the 800 ground candidates of the seeded fit) with `count` pixels of the rows above the
    horizon overwritten by returns on the pixels' own rays at ranges 1e6 * growth^j: float32 [N,3].  The base points of those columns are
    removed as the builder removes those of its row-end columns; the columns differ from scene to scene."""
    H, W, _, _, count, growth = C_FORMS[form]
    rows = c_rows(H)
    per = -(-count // len(rows))
    stride = max((W - 12) // per, 1)
    cols = 4 + k + stride * np.arange(per)
    assert cols[-1] < W - 4 and per * len(rows) >= count
    f = lv.scene_frame(H, W, k)
    az = np.mod(np.arctan2(f[:, 1].astype(np.float64), f[:, 0].astype(np.float64)), 2 * np.pi) / (2 * np.pi) * W
    el = np.degrees(np.arctan2(f[:, 2].astype(np.float64), np.hypot(f[:, 0].astype(np.float64), f[:, 1].astype(np.float64))))
    hrow = (el - lv.VMIN_DEG) / (lv.VMAX_DEG - lv.VMIN_DEG) * (H - 1)
    near_col = np.abs(az[:, None] - cols[None, :]).min(1) < 1.0
    f = f[~(near_col & (hrow > rows[0] - 1.0))]
    hh, cc = np.meshgrid(np.asarray(rows), cols, indexing="ij")
    hh, cc = hh.reshape(-1)[:count], cc.reshape(-1)[:count]
    r = C_R0 * growth ** np.arange(count, dtype=np.float64)
    e, a = np.radians(lv.VMIN_DEG + (lv.VMAX_DEG - lv.VMIN_DEG) * hh / (H - 1)), 2 * np.pi * cc / W
    far = np.stack([r * np.cos(e) * np.cos(a), r * np.cos(e) * np.sin(a), r * np.sin(e)], -1).astype(F32)
    out = np.ascontiguousarray(np.concatenate([f, far]))
    out.setflags(write=False)
    return out, (hh, cc, r)
