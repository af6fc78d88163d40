"""-m gpu: the point model's range sums added by assign_kernel, and the count-only label histogram beside it, in the fused batch.

Every case is a small batch through ops.compress_batch (or the mixed call) whose outputs -- labels, counts, nnz, model rows including
the NaN rows of labels without pixels, quantised integers -- are compared bit for bit with the CPU oracle.  The scenes and what each
is there for: tests/assign_sums_cases.py (checked on the CPU by tests/test_assign_sums_cases.py)."""
import numpy as np
import pytest

import assign_sums_cases as ac

pytestmark = pytest.mark.gpu


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


def _beq(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _np(t):
    return t.cpu().numpy()


def _group(env, name, buf=None):
    """compress_batch's arguments for a case: its frames, the injected ground plane, buffers of its shape (or `buf`)."""
    torch, ops = env["torch"], env["ops"]
    H, W, M, _ = ac.CASES[name]
    g, tm = ac.shape(H, W)
    assert np.array_equal(ops.transform_map(g.H, g.W, g.horizontal_FOV, g.vertical_max, g.vertical_min), tm)
    frames = ac.case_frames(name)
    B = len(frames)
    offs = np.zeros(B + 1, np.int64)
    offs[1:] = np.cumsum([f.shape[0] for f in frames])
    if buf is None:
        buf = ops.BatchBuffers(B, ops.make_geom(g.H, g.W, g.horizontal_FOV, g.vertical_max, g.vertical_min), M, env["dev"])
    assert (buf.B, buf.P, buf.M) == (B, H * W, M)
    return dict(xyz=_to(env, np.concatenate(frames)), offsets=_to(env, offs), tm=_to(env, tm), ground=_to(env, np.tile(ac.GROUND, (B, 1))), buf=buf)


def _check(buf, exp, tag):
    """Every frame's outputs against the oracle's."""
    ri, seg, pix, cen = _np(buf.ri), _np(buf.seg), _np(buf.cen_pix), _np(buf.centers)
    q, nz, mo, cnt = _np(buf.q16), _np(buf.nnz), _np(buf.model), _np(buf.counts)
    for i, e in enumerate(exp):
        nrow = e["model"].shape[0]
        assert _beq(ri[i], e["ri"]), (tag, i, "range image")
        assert np.array_equal(pix[i], e["pix"]) and _beq(cen[i], e["cen"]), (tag, i, "centres")
        assert np.array_equal(seg[i].astype(np.int64), e["seg"]), (tag, i, "labels")
        assert np.array_equal(cnt[i], e["counts"]), (tag, i, "counts", cnt[i], e["counts"])
        assert _beq(mo[i, :nrow], e["model"]), (tag, i, "model rows", mo[i, :nrow, 3], e["model"][:, 3])
        # (the oracle's table ends at the largest label a pixel carries: the rows behind it are labels without pixels)
        assert (mo[i, nrow:, 3].view(np.uint32) == ac.NAN_ROW).all() and not mo[i, nrow:, :3].any(), (tag, i, "rows of unused labels")
        for lab in ac.empty_labels(e):
            assert mo[i, lab, 3].view(np.uint32) == ac.NAN_ROW, (tag, i, lab)
        assert int(nz[i]) == e["q"].shape[0] and np.array_equal(q[i, :nz[i]], e["q"]), (tag, i, "quantised integers")


def _inexact_flags(buf):
    """The frames' "a range left the fixed-point window" flags, from the model part that opens the workspace: sums i64 [B][KP] | flags
    i32 [B][4] (ws_layout, rpcc_hip.hip)."""
    off = buf.B * ac.kpad(buf.M) * 8
    return _np(buf.ws[off:off + buf.B * 16]).view(np.int32).reshape(buf.B, 4)[:, 0]


def _run(env, name):
    a = _group(env, name)
    env["ops"].compress_batch(**a)
    env["torch"].cuda.synchronize()
    return a["buf"]


@pytest.mark.parametrize("name", ["ragged", "vector", "w2250", "scalar", "packed", "uint16"])
def test_fused_batch_equals_the_oracle(env, name):
    """ragged: partial tiles, a padding wavefront, one ragged scatter tile, three scenes in one call.  vector / w2250 / scalar: the 4-pixel and
    the element-wise form of the count-only histogram.  packed: twelve cluster labels in one tile (the aggregation loop past three rounds)
    and a label without pixels.  uint16: uint16 labels, with a label without pixels."""
    buf = _run(env, name)
    assert buf.seg.dtype == (env["torch"].uint16 if name == "uint16" else env["torch"].uint8)
    _check(buf, ac.case_expected(name), name)
    assert not _inexact_flags(buf).any(), name


def test_ranges_outside_the_fixed_point_window(env):
    """The middle frame has cluster pixels below 2^-5 m and at or above 2^8 m: its flag is set and its rows are the oracle's sequential
    sums; the frames around it keep their flags clear and their fixed-point rows."""
    buf = _run(env, "window")
    assert _inexact_flags(buf).tolist() == [0, 1, 0]
    _check(buf, ac.case_expected("window"), "window")


def test_two_calls_on_one_workspace(env):
    """A workspace filled with a pattern, then two calls with different frames: neither the pattern nor the first call's sums and flag
    reach the second call's rows."""
    a = _group(env, "window")
    a["buf"].ws.fill_(0xA5)
    env["ops"].compress_batch(**a)
    env["torch"].cuda.synchronize()
    assert _inexact_flags(a["buf"]).tolist() == [0, 1, 0]
    _check(a["buf"], ac.case_expected("window"), "first call")
    b = _group(env, "reuse", buf=a["buf"])
    env["ops"].compress_batch(**b)
    env["torch"].cuda.synchronize()
    assert _inexact_flags(b["buf"]).tolist() == [0, 0, 0]
    _check(b["buf"], ac.case_expected("reuse"), "second call")


def test_mixed_call_equals_its_groups_alone(env):
    """Two geometry groups in one rpcc_compress_batch_mixed (the second takes the element-wise histogram form; the first holds the frame
    outside the window): every group equals the same group through rpcc_compress_batch, and the oracle."""
    ops = env["ops"]
    names = [n for n, _, _ in ac.MIXED]
    alone = [_group(env, n) for n in names]
    for a in alone:
        ops.compress_batch(**a)
    mixed = [_group(env, n) for n in names]
    ops.compress_batch_mixed(mixed)
    env["torch"].cuda.synchronize()
    for n, a, m in zip(names, alone, mixed):
        for f in ("ri", "seg", "cen_pix", "centers", "model", "counts", "nnz"):
            assert _beq(_np(getattr(a["buf"], f)), _np(getattr(m["buf"], f))), (n, f)
        _check(m["buf"], ac.case_expected(n), ("mixed", n))
        assert np.array_equal(_inexact_flags(m["buf"]), _inexact_flags(a["buf"])), n
    assert _inexact_flags(mixed[0]["buf"]).tolist() == [0, 1, 0] and not _inexact_flags(mixed[1]["buf"]).any()


def test_single_stage_entries_equal_the_fused_result(env):
    """rpcc_assign (labels only) and rpcc_point_model (the histogram with sums) on the fused call's range images and centres."""
    ops = env["ops"]
    a = _group(env, "window")
    buf = ops.compress_batch(**a)
    seg = ops.assign(buf.ri, a["tm"], a["ground"], buf.centers)
    model, counts = ops.point_model(buf.ri, seg, a["ground"], buf.M)
    env["torch"].cuda.synchronize()
    assert _beq(_np(seg), _np(buf.seg)) and _beq(_np(model), _np(buf.model)) and _beq(_np(counts), _np(buf.counts))
    _check(buf, ac.case_expected("window"), "fused")
