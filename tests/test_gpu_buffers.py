"""-m gpu: the caller-buffer contract of the five libraries (the "Caller's buffers" paragraphs of include/*.h).

Every workspace, scratch buffer and table here is an Arena view (tests/buffer_arena.py) of EXACTLY the bytes the library's size function
returns -- no rounding up --, filled with a hostile pattern and surrounded by guard bytes; every result is compared with the CPU oracle bit
for bit, and the guards must come back untouched.  The batches are those of tests/buffer_cases.py (tests/test_buffer_cases.py proves what
they cross).  test_*_unwritten_* list the output bytes a call leaves alone and hold the list to what the headers declare.

Entry points that take a caller's work buffer, and the test that hands each an arena:
  rpcc_compress_batch (rpcc_workspace_bytes / _general)  test_fused_batch_on_poisoned_workspace, test_workspace_reused_under_another_layout,
                                                         test_fused_batch_unwritten_bytes
  rpcc_compress_batch_wide (rpcc_wide_workspace_bytes)   the same tests at cluster_num 300 (tuned kernels on uint16 labels) and 1100 (radix sort)
  rpcc_compress_batch_mixed                              test_mixed_batch_on_poisoned_workspaces
  rpcc_compress_batch_stages                             test_stages_one_bit_per_call_on_poisoned_workspace
  ops.compress_batch_general (the staged front-end)      test_staged_general_on_poisoned_workspace (buf.ws of rpcc_workspace_bytes_general bytes)
  rpcc_project / rpcc_project_strided                    test_project_scratch (both paths; ops.project goes through the strided entry)
  rpcc_ground_mask -> rpcc_fps_range (fps_table)         test_fps_table
  rpcc_point_model[_wide], rpcc_predict_quantize[_wide]  test_point_model_and_quantiser_workspace
  rpcc_plane_model[_wide]                                test_plane_model_workspace
  rpcc_contour_encode / _decode, rpcc_decode [_wide]     test_codec_workspace
  rpcc_seg_dbscan                                        test_dbscan_workspace
  rpcc_eval_nn / _normals / _metrics                     test_eval_workspace
  rpcc_lz4_encode / _decode / _pack_containers           test_lz4_buffers (the first two take no work buffer: their output slots are the arena)
  rpcc_deflate_encode                                    test_deflate_workspace
Which output bytes a call leaves alone: test_fused_batch_unwritten_bytes (the fused entries), test_stage_entries_unwritten_bytes (projection,
mask + FPS, both models, quantiser, rpcc_pack_payload, contour codec, decoder), test_side_libraries_unwritten_bytes (DBSCAN, the three eval
entries) and test_entropy_coders_unwritten_bytes (rpcc_deflate_encode, rpcc_lz4_encode / _decode / _pack_containers, a refused stream and a
failed container among them).  The tests use 256-byte aligned buffers; test_work_buffers_at_the_stated_alignment runs one case of every
library at the smaller alignment its header states (base + 16, base + 8 for the entropy coders)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import buffer_cases as BC   # noqa: E402
from buffer_arena import PATTERNS, Arena, filled, unwritten   # noqa: E402

STAGE_PATTERNS = ("zero", "ones", "nan", "alt(0,0)", "alt(0,1)", "half(0)", "half(1)")
SIDE_PATTERNS = ("zero", "ones", "alt(0,0)", "alt(0,1)", "half(0)", "half(1)")
POISON = 0xCD          # what output buffers hold before a call whose result is compared


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    import rpcc_amd  # noqa: F401
    from rpcc_amd import _lib, ops
    from oracle import oracle as orc
    return dict(torch=torch, ops=ops, lib=_lib, orc=orc, dev=torch.device("cuda:0"), cache={})


def _to(env, a):
    return env["torch"].from_numpy(np.ascontiguousarray(a)).to(env["dev"])


def _beq(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _clean(arena, what):
    bad = arena.check_guards()
    assert bad is None, "%s: bytes outside the buffer of %d bytes were written, offsets %d .. %d relative to its start" % ((what, arena.nbytes) + bad)


# ------------------------------------------------------------------------------------------------
# the cases on the device
# ------------------------------------------------------------------------------------------------
def _inputs(env, name, scene, nframes=BC.B):
    """Device inputs of the first nframes frames of a geometry (shared by every test: never written)."""
    key = (name, scene, nframes)
    if key not in env["cache"]:
        ops, orc = env["ops"], env["orc"]
        g = BC.geom_of(name)
        tm = ops.transform_map(g.H, g.W, g.horizontal_FOV, g.vertical_max, g.vertical_min)
        assert np.array_equal(tm, orc.transform_map(g))
        fr = BC.frames(name, scene)[:nframes]
        env["cache"][key] = dict(g=g, geom=ops.make_geom(g.H, g.W, g.horizontal_FOV, g.vertical_max, g.vertical_min), tm_np=tm, tm=_to(env, tm),
                                 frames=fr, xyz=_to(env, np.concatenate(fr)), offs=_to(env, BC.offsets(fr)), total=int(sum(f.shape[0] for f in fr)),
                                 P=g.H * g.W, B=nframes)
    return env["cache"][key]


def _ws_bytes(env, inp, M, variant):
    lib = env["lib"].lib()
    fn = lib.rpcc_wide_workspace_bytes if M > env["lib"].MAX_CLUSTERS else lib.rpcc_workspace_bytes if variant == "uniform_point" else lib.rpcc_workspace_bytes_general
    n = int(fn(inp["B"], inp["P"], M, inp["total"]))
    assert n > 0
    return n


def _buffers(env, inp, M, variant, ws):
    """BatchBuffers whose work buffer is `ws` (exact size: ops.workspace's round-up is bypassed) and whose outputs hold POISON."""
    torch, ops = env["torch"], env["ops"]
    buf = ops.BatchBuffers(inp["B"], inp["geom"], M, env["dev"], max_points=inp["total"], general=variant != "uniform_point")
    buf.ws = ws
    if buf.salience is None:      # (uniform / point, byte labels: the front-end allocates neither; the tests want to see them left alone)
        buf.salience = torch.empty((inp["B"], M + 2), dtype=torch.uint8, device=env["dev"])
        buf.key_point_map = torch.empty((inp["B"], inp["g"].H, inp["g"].W), dtype=torch.uint8, device=env["dev"])
    _poison(buf, POISON)
    return buf


OUTPUTS = ("ri", "seg", "cen_pix", "centers", "model", "counts", "q16", "nnz", "info", "salience", "key_point_map")


def _poison(buf, byte):
    import torch
    for f in OUTPUTS:
        getattr(buf, f).reshape(-1).view(torch.uint8).fill_(byte)


def _kw(env, M, variant):
    ops = env["ops"]
    uniform = variant == "uniform_point"
    return dict(ground_threshold=BC.GROUND_THRESHOLD, acc=BC.ACC, ground_seed=BC.GROUND_SEED, model_method="point" if uniform else "plane",
                angle_threshold=BC.ANGLE, plane_seed=BC.PLANE_SEED, nonuniform=None if uniform else ops.nonuniform_cfg(BC.ACC, BC.oracle_cfg(M)))


def _ground_out(env, B):
    return filled((B, 4), env["torch"].float64, env["dev"], POISON)


def _check(env, inp, buf, gfit, exp, M, variant, tag, salience=None, key_points=True):
    """Every output of the fused call against the oracle, every frame: no frame is skipped.  salience: the levels where the call returns them
    instead of filling buf.salience; key_points=False: the call does not hand out its key-point map (both: ops.compress_batch_general)."""
    torch = env["torch"]
    torch.cuda.synchronize()
    P, K = inp["P"], M + 2
    out = {f: getattr(buf, f).cpu().numpy() for f in OUTPUTS}
    gf = gfit.cpu().numpy()
    sal = out["salience"] if salience is None else salience.cpu().numpy()
    for b in range(inp["B"]):
        t = tag + (b, BC.KINDS[b])
        o = exp[b]
        if o is None:       # the sweep without points: an empty image, every pixel label 1, no payload
            assert not out["ri"][b].any() and (out["seg"][b] == 1).all() and out["nnz"][b] == 0, t
            want = np.zeros(K, np.int32)
            want[1] = P
            assert np.array_equal(out["counts"][b], want), t
            continue
        assert _beq(gf[b], o["ground"]), (t, "ground")
        assert _beq(out["ri"][b], o["range_image"]), (t, "ri")
        assert np.array_equal(out["cen_pix"][b], o["fps_pix"]), (t, "cen_pix")
        bad = np.flatnonzero(out["seg"][b].reshape(-1) != o["seg_idx"].reshape(-1))
        assert bad.size == 0, (t, "seg", bad[:6])
        mp = np.asarray(o["model_param"]).astype(np.float32)
        rows = mp.shape[0]
        assert _beq(out["model"][b, :rows], mp), (t, "model")
        assert np.array_equal(out["counts"][b, :rows], np.bincount(o["seg_idx"].reshape(-1), minlength=rows)), (t, "counts")
        n = int(out["nnz"][b])
        assert n == o["q"].shape[0], (t, "nnz", n, o["q"].shape[0])
        assert np.array_equal(out["q16"][b, :n], o["q"].astype(np.int16)), (t, "q16")
        if variant.startswith("nonuniform"):
            if key_points:
                assert np.array_equal(out["key_point_map"][b], o["key_point_map"].astype(np.uint8)), (t, "key_point_map")
            assert np.array_equal(sal[b, :o["salience"].shape[0]], o["salience"].astype(np.uint8)), (t, "salience")


FUSED = [(n, M, v) for n in BC.GEOMETRIES for M in BC.CLUSTERS[n] for v in BC.VARIANTS]


# ------------------------------------------------------------------------------------------------
# a. the fused entries: workspace contents do not matter, nothing is written outside
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,M,variant", FUSED)
def test_fused_batch_on_poisoned_workspace(env, name, M, variant):
    """rpcc_compress_batch (uniform / point: rpcc_workspace_bytes; non-uniform / plane: rpcc_workspace_bytes_general) and rpcc_compress_batch_wide
    (cluster_num 300: the tuned kernels on uint16 labels; 1100: the radix-sort kernels) on a workspace of exactly the declared size under every
    pattern: all outputs equal the oracle's, the guards stay clean.  The alt patterns force a stale projection flag to equal the call's mark."""
    ops = env["ops"]
    inp = _inputs(env, name, BC.scene_of(M))
    exp = BC.expected(name, M, variant)
    arena = Arena(_ws_bytes(env, inp, M, variant), env["dev"])
    kw = _kw(env, M, variant)
    for pattern in PATTERNS:
        arena.fill(pattern)
        buf = _buffers(env, inp, M, variant, arena.view)
        gfit = _ground_out(env, inp["B"])
        ops.compress_batch(inp["xyz"], inp["offs"], inp["tm"], gfit, buf, **kw)
        _check(env, inp, buf, gfit, exp, M, variant, (name, M, variant, pattern))
        _clean(arena, "compress_batch %s M=%d %s, workspace %s" % (name, M, variant, pattern))
        assert buf.ws.data_ptr() == arena.view.data_ptr()      # (the front-end did not swap the workspace for a larger one)


@pytest.mark.parametrize("variants", [("uniform_point", "uniform_point"), ("nonuniform_plane", "uniform_point"), ("uniform_point", "nonuniform_plane")])
def test_mixed_batch_on_poisoned_workspaces(env, variants):
    """rpcc_compress_batch_mixed, two geometry groups (5 x 300 and 16 x 1800) with a workspace arena each."""
    ops = env["ops"]
    M = 100
    names = ("5x300", "16x1800")
    inps = [_inputs(env, n, "default") for n in names]
    exps = [BC.expected(n, M, v) for n, v in zip(names, variants)]
    arenas = [Arena(_ws_bytes(env, i, M, v), env["dev"]) for i, v in zip(inps, variants)]
    for pattern in PATTERNS:
        groups = []
        for inp, v, a in zip(inps, variants, arenas):
            a.fill(pattern)
            kw = _kw(env, M, v)
            kw.pop("ground_threshold"), kw.pop("acc")
            groups.append(dict(xyz=inp["xyz"], offsets=inp["offs"], tm=inp["tm"], ground=_ground_out(env, inp["B"]), buf=_buffers(env, inp, M, v, a.view), **kw))
        ops.compress_batch_mixed(groups, ground_threshold=BC.GROUND_THRESHOLD, acc=BC.ACC)
        for n, inp, v, a, gr, exp in zip(names, inps, variants, arenas, groups, exps):
            _check(env, inp, gr["buf"], gr["ground"], exp, M, v, ("mixed", n, v, pattern))
            _clean(a, "compress_batch_mixed group %s %s, workspace %s" % (n, v, pattern))


class _Settings:      # what ops.compress_batch_general reads of a pipeline.BatchCompressor
    pass


@pytest.mark.parametrize("name,M,variant", [("5x300", 100, "nonuniform_plane"), ("5x300", 100, "nonuniform_point"), ("16x2101", 100, "nonuniform_plane"),
                                            ("16x2101", 100, "nonuniform_point")])
def test_staged_general_on_poisoned_workspace(env, name, M, variant):
    """ops.compress_batch_general, the staged front-end of the plane model / non-uniform framework, with buf.ws an arena of exactly
    rpcc_workspace_bytes_general(B, P, M, total) bytes: it hands buf.ws to rpcc_point_model and rpcc_predict_quantize (its other temporaries are
    its own allocations).  The oracle's ground planes go in (fit_ground=False: the staged path draws the ground and the plane fits from ONE
    seed, the cases use two); every output it fills equals the oracle's, the returned salience levels included."""
    ops = env["ops"]
    inp = _inputs(env, name, "default")
    exp = BC.expected(name, M, variant)
    arena = Arena(int(env["lib"].lib().rpcc_workspace_bytes_general(inp["B"], inp["P"], M, inp["total"])), env["dev"])
    cc = _Settings()
    cc.seed, cc.ground_threshold, cc.acc, cc.cfg = BC.PLANE_SEED, BC.GROUND_THRESHOLD, BC.ACC, BC.oracle_cfg(M)
    cc.uniform, cc.model_method = variant.startswith("uniform"), variant.split("_")[1]
    ground = np.stack([EMPTY_GROUND if o is None else o["ground"] for o in exp])
    for pattern in ("ones", "alt(0,0)", "alt(0,1)", "half(0)", "half(1)"):
        arena.fill(pattern)
        buf = _buffers(env, inp, M, "nonuniform_plane", arena.view)
        gfit = _to(env, ground)
        sal = ops.compress_batch_general(inp["xyz"], inp["offs"], inp["tm"], gfit, buf, cc, False)
        assert buf.ws.data_ptr() == arena.view.data_ptr()
        _check(env, inp, buf, gfit, exp, M, variant, ("general", name, M, variant, pattern), salience=sal, key_points=False)
        _clean(arena, "compress_batch_general %s M=%d %s, workspace %s" % (name, M, variant, pattern))


# ------------------------------------------------------------------------------------------------
# b. stage by stage on one poisoned workspace
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,M,variant", [("5x300", 7, "uniform_point"), ("5x300", 100, "nonuniform_plane"), ("16x2101", 100, "nonuniform_plane"),
                                            ("16x2101", 254, "uniform_point"), ("16x1800", 100, "uniform_point"), ("16x1800", 7, "nonuniform_plane")])
def test_stages_one_bit_per_call_on_poisoned_workspace(env, name, M, variant):
    """rpcc_compress_batch_stages with one stage bit per call (1, 2, 4 .. 64): what a stage needs of the workspace is what the stages before it
    left there, whatever the workspace held before the first one."""
    ops = env["ops"]
    inp = _inputs(env, name, "default")
    exp = BC.expected(name, M, variant)
    arena = Arena(_ws_bytes(env, inp, M, variant), env["dev"])
    kw = _kw(env, M, variant)
    for pattern in ("ones", "alt(0,0)", "alt(0,1)", "half(0)", "half(1)"):
        arena.fill(pattern)
        buf = _buffers(env, inp, M, variant, arena.view)
        gfit = _ground_out(env, inp["B"])
        for bit in range(7):
            ops.compress_batch_stages(1 << bit, inp["xyz"], inp["offs"], inp["tm"], gfit, buf, **kw)
        _check(env, inp, buf, gfit, exp, M, variant, ("stages", name, M, variant, pattern))
        _clean(arena, "compress_batch_stages %s M=%d %s, workspace %s" % (name, M, variant, pattern))


# ------------------------------------------------------------------------------------------------
# c. one workspace reused under other layouts
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["zero", "ones", "alt(0,0)", "alt(0,1)", "half(0)", "half(1)"])
def test_workspace_reused_under_another_layout(env, pattern):
    """What BatchBuffers / StreamingCompressor do: one allocation serves calls of different shapes.  X (16 x 2101, M = 100), Y (5 x 300, M = 7,
    general), X again, Y with three frames -- no refill in between, so every call reads the mark and the flag words out of what a call under
    another layout left behind.  Each call gets the arena's first bytes(case) bytes and must not touch the rest."""
    torch, ops = env["torch"], env["ops"]
    X = ("16x2101", 100, "uniform_point", BC.B)
    Y = ("5x300", 7, "nonuniform_plane", BC.B)
    Y3 = ("5x300", 7, "nonuniform_plane", 3)
    calls = [X, Y, X, Y3]
    need = [_ws_bytes(env, _inputs(env, n, "default", nf), M, v) for n, M, v, nf in calls]
    arena = Arena(max(need), env["dev"]).fill(pattern)
    for k, ((name, M, variant, nf), n) in enumerate(zip(calls, need)):
        inp = _inputs(env, name, "default", nf)
        rest = arena.view[n:].clone()
        buf = _buffers(env, inp, M, variant, arena.first(n))
        gfit = _ground_out(env, nf)
        ops.compress_batch(inp["xyz"], inp["offs"], inp["tm"], gfit, buf, **_kw(env, M, variant))
        _check(env, inp, buf, gfit, BC.expected(name, M, variant)[:nf], M, variant, ("reuse", pattern, k, name))
        assert torch.equal(arena.view[n:], rest), ("reuse", pattern, k, "bytes past the %d the call was given were written" % n)
        _clean(arena, "reuse call %d" % k)


# ------------------------------------------------------------------------------------------------
# d. the stage entries that take a buffer
# ------------------------------------------------------------------------------------------------
EMPTY_GROUND = np.array([0.0, 0.0, 1.0, 1.7])      # the plane handed in for the sweep without points (no fit is defined for it)
STAGE_CASES = [("5x300", 100), ("16x2101", 100), ("16x1800", 300)]      # 300: the `_wide` forms


def _stage_inputs(env, name, M):
    """The oracle's intermediates of a case as device tensors, the empty frame filled in with what an empty image is (labels 1)."""
    key = ("stage", name, M)
    if key in env["cache"]:
        return env["cache"][key]
    torch = env["torch"]
    inp = _inputs(env, name, "default")
    eu, ep = BC.expected(name, M, "uniform_point"), BC.expected(name, M, "nonuniform_plane")
    g, P, K, B = inp["g"], inp["P"], M + 2, inp["B"]
    ri = np.zeros((B, g.H, g.W), np.float32)
    seg = np.ones((B, g.H, g.W), np.uint16 if M > 254 else np.uint8)
    ground = np.tile(EMPTY_GROUND, (B, 1))
    model_u, model_p = np.zeros((B, K, 4), np.float32), np.zeros((B, K, 4), np.float32)
    for b in range(B):
        if eu[b] is None:
            continue
        ri[b], seg[b], ground[b] = eu[b]["range_image"], eu[b]["seg_idx"], eu[b]["ground"]
        for m, e in ((model_u, eu), (model_p, ep)):
            mp = np.asarray(e[b]["model_param"]).astype(np.float32)
            m[b, :mp.shape[0]] = mp
        assert np.array_equal(eu[b]["seg_idx"], ep[b]["seg_idx"])
    d = dict(inp=inp, eu=eu, ep=ep, ri=_to(env, ri), seg=_to(env, seg), ground=_to(env, ground), model_u=_to(env, model_u), model_p=_to(env, model_p),
             seg_np=seg, model_u_np=model_u, model_p_np=model_p, live=[b for b in range(B) if eu[b] is not None])
    env["cache"][key] = d
    return d


@pytest.mark.parametrize("atomic", [False, True])
@pytest.mark.parametrize("name", sorted(BC.GEOMETRIES))
def test_project_scratch(env, name, atomic):
    """rpcc_project: the LDS-band path on rpcc_project_scratch_bytes(total, B, P) bytes, the device-atomic path on B * (P + 8) * 4."""
    ops = env["ops"]
    inp = _inputs(env, name, "default")
    ris, _ = BC.grounds(name, "default")
    n = inp["B"] * (inp["P"] + 8) * 4 if atomic else int(env["lib"].lib().rpcc_project_scratch_bytes(inp["total"], inp["B"], inp["P"]))
    arena = Arena(n, env["dev"])
    for pattern in STAGE_PATTERNS:
        arena.fill(pattern)
        out = filled((inp["B"], inp["g"].H, inp["g"].W), env["torch"].float32, env["dev"], POISON)
        ri = ops.project(inp["xyz"], inp["offs"], inp["geom"], ri=out, scratch=arena.view, atomic_path=atomic).cpu().numpy()
        for b in range(inp["B"]):
            assert _beq(ri[b], ris[b]), (name, atomic, pattern, b, BC.KINDS[b])
        _clean(arena, "project %s atomic=%s scratch %s" % (name, atomic, pattern))


@pytest.mark.parametrize("name,M", STAGE_CASES)
def test_fps_table(env, name, M):
    """rpcc_ground_mask's tile table (rpcc_fps_table_bytes) handed on to rpcc_fps_range."""
    ops = env["ops"]
    s = _stage_inputs(env, name, M)
    inp = s["inp"]
    g = inp["g"]
    arena = Arena(int(env["lib"].lib().rpcc_fps_table_bytes(inp["B"], g.H, g.W)), env["dev"])
    for pattern in STAGE_PATTERNS:
        arena.fill(pattern)
        temp, info, tab = ops.ground_mask(s["ri"], inp["tm"], s["ground"], BC.GROUND_THRESHOLD, fps_table=True, table=arena.view)
        cen_pix, centers = ops.fps_range(s["ri"], inp["tm"], temp, info, M, fps_table=tab)
        cen_pix, centers, info = cen_pix.cpu().numpy(), centers.cpu().numpy(), info.cpu().numpy()
        for b in s["live"]:
            o = s["eu"][b]
            assert info[b, 0] == int(o["mask"].sum()) and info[b, 1] == np.flatnonzero(o["mask"].reshape(-1))[0], (name, pattern, b)
            assert np.array_equal(cen_pix[b], o["fps_pix"]), (name, pattern, b)
            assert _beq(centers[b], o["centers"]), (name, pattern, b)
        _clean(arena, "fps table %s M=%d, %s" % (name, M, pattern))


@pytest.mark.parametrize("name,M", STAGE_CASES)
def test_point_model_and_quantiser_workspace(env, name, M):
    """rpcc_point_model / rpcc_predict_quantize (and their _wide forms at M = 300) on rpcc_workspace_bytes(B, P, M, 0) bytes."""
    ops, torch = env["ops"], env["torch"]
    s = _stage_inputs(env, name, M)
    inp = s["inp"]
    arena = Arena(int(env["lib"].lib().rpcc_workspace_bytes(inp["B"], inp["P"], M, 0)), env["dev"])
    for pattern in STAGE_PATTERNS:
        arena.fill(pattern)
        model, counts = ops.point_model(s["ri"], s["seg"], s["ground"], M, ws=arena.view)
        _clean(arena, "point_model %s M=%d, %s" % (name, M, pattern))
        model, counts = model.cpu().numpy(), counts.cpu().numpy()
        arena.fill(pattern)
        q_out = filled((inp["B"], inp["P"]), torch.int16, env["dev"], POISON)
        q, nnz, pred = ops.predict_quantize(s["ri"], inp["tm"], s["seg"], s["model_u"], BC.ACC, M, want_pred=True, int16=True, ws=arena.view, q_out=q_out)
        _clean(arena, "predict_quantize %s M=%d, %s" % (name, M, pattern))
        q, nnz, pred = q.cpu().numpy(), nnz.cpu().numpy(), pred.cpu().numpy()
        for b in s["live"]:
            o = s["eu"][b]
            rows = o["model_param"].shape[0]
            assert _beq(model[b, :rows], s["model_u_np"][b, :rows]), (name, pattern, b)
            assert np.array_equal(counts[b, :rows], np.bincount(o["seg_idx"].reshape(-1), minlength=rows)), (name, pattern, b)
            assert nnz[b] == o["q"].shape[0] and np.array_equal(q[b, :nnz[b]], o["q"].astype(np.int16)), (name, pattern, b)
            assert _beq(pred[b].reshape(o["pred"].shape), o["pred"]), (name, pattern, b)


@pytest.mark.parametrize("name,M", STAGE_CASES)
def test_plane_model_workspace(env, name, M):
    """rpcc_plane_model (_wide at M = 300) on rpcc_plane_workspace_bytes(B, P, M) bytes: its label scan clears its own sums."""
    ops = env["ops"]
    s = _stage_inputs(env, name, M)
    inp = s["inp"]
    arena = Arena(int(env["lib"].lib().rpcc_plane_workspace_bytes(inp["B"], inp["P"], M)), env["dev"])
    for pattern in STAGE_PATTERNS:
        arena.fill(pattern)
        model, counts = ops.plane_model(s["ri"], inp["tm"], s["seg"], M, angle_threshold=BC.ANGLE, seed=BC.PLANE_SEED, ground=s["ground"], want_counts=True,
                                        ws=arena.view)
        model, counts = model.cpu().numpy(), counts.cpu().numpy()
        for b in s["live"]:
            o = s["ep"][b]
            rows = o["model_param"].shape[0]
            assert _beq(model[b, :rows], s["model_p_np"][b, :rows]), (name, pattern, b)
            assert np.array_equal(counts[b, :rows], np.bincount(o["seg_idx"].reshape(-1), minlength=rows)), (name, pattern, b)
        _clean(arena, "plane_model %s M=%d, %s" % (name, M, pattern))


def _dequantise(o, step):
    """QuantizationModule.dequantize_residual, uniform (utils/compress_utils.py:114-132) on the oracle's label map and integers."""
    seg = o["seg_idx"]
    q = o["q"].astype(np.int16)
    res = np.zeros(seg.shape, np.float32)
    start = 0
    for m in range(int(seg.max()) + 1):
        if m == 1:
            continue
        idx = np.where(seg == m)
        res[idx] = q[start:start + idx[0].shape[0]] * step
        start += idx[0].shape[0]
    assert start == q.shape[0]
    return np.expand_dims(res, -1)


def _codec_bytes(env, inp, M):
    lib = env["lib"].lib()
    return int(lib.rpcc_wide_workspace_bytes(inp["B"], inp["P"], M, 0) if M > env["lib"].MAX_CLUSTERS else lib.rpcc_codec_workspace_bytes(inp["B"], inp["P"], M))


@pytest.mark.parametrize("name,M", STAGE_CASES)
def test_codec_workspace(env, name, M):
    """rpcc_contour_encode / rpcc_contour_decode / rpcc_decode (_wide at M = 300) on the codec workspace: the oracle's contour bits and index
    sequence, the label map back, and the reference decoder's arithmetic."""
    ops, orc, torch = env["ops"], env["orc"], env["torch"]
    s = _stage_inputs(env, name, M)
    inp = s["inp"]
    g, B, P = inp["g"], inp["B"], inp["P"]
    arena = Arena(_codec_bytes(env, inp, M), env["dev"])
    q16 = np.zeros((B, P), np.int16)
    for b in s["live"]:
        q16[b, :s["eu"][b]["q"].shape[0]] = s["eu"][b]["q"]
    d_q16 = _to(env, q16)
    want = {}
    for b in range(B):
        cm, sq = orc.extract_contour(s["seg_np"][b].astype(np.int32))
        want[b] = (np.packbits(cm.astype(bool), axis=None), sq.astype(np.uint16))
    for pattern in STAGE_PATTERNS:
        arena.fill(pattern)
        bits, seq, nseq = ops.contour_encode(s["seg"], M, ws=arena.view)
        _clean(arena, "contour_encode %s M=%d, %s" % (name, M, pattern))
        arena.fill(pattern)
        seg_rec = ops.contour_decode(bits, seq, g.H, g.W, M, ws=arena.view)
        _clean(arena, "contour_decode %s M=%d, %s" % (name, M, pattern))
        arena.fill(pattern)
        rec, pc = ops.decode(seg_rec, d_q16, s["model_u"], inp["tm"], BC.ACC, want_points=True, ws=arena.view)
        _clean(arena, "decode %s M=%d, %s" % (name, M, pattern))
        bits, seq, nseq, seg_rec, rec, pc = (t.cpu().numpy() for t in (bits, seq, nseq, seg_rec, rec, pc))
        assert np.array_equal(seg_rec, s["seg_np"]), (name, pattern)
        for b in range(B):
            assert nseq[b] == want[b][1].shape[0] and np.array_equal(seq[b, :nseq[b]], want[b][1]), (name, pattern, b)
            assert np.array_equal(bits[b], want[b][0]), (name, pattern, b)
        for b in s["live"]:
            o = s["eu"][b]
            e = o["pred"] + _dequantise(o, BC.ACC)
            assert _beq(rec[b].reshape(e.shape), e), (name, pattern, b)
            assert _beq(pc[b], e * inp["tm_np"]), (name, pattern, b)


# ------------------------------------------------------------------------------------------------
# e. the side libraries
# ------------------------------------------------------------------------------------------------
def test_dbscan_workspace(env):
    """rpcc_seg_dbscan (16 x 1800, two frames, eps 0.45) on rpcc_seg_workspace_bytes: the brute-force run on a zeroed workspace, and the numpy
    reference for the first frame."""
    torch = env["torch"]
    import dbscan_ref
    from rpcc_amd import _seg_lib, dbscan
    inp = _inputs(env, "16x1800", "default")
    ris, gms = BC.grounds("16x1800", "default")
    pick = [0, 1]
    ri = _to(env, np.stack([ris[b] for b in pick]))
    ground = _to(env, np.stack([gms[b] for b in pick]))
    tm3 = inp["tm"].reshape(inp["g"].H, inp["g"].W, 3)
    arena = Arena(int(_seg_lib.lib().rpcc_seg_workspace_bytes(2, inp["g"].H, inp["g"].W)), env["dev"])
    arena.fill("zero")
    ref_seg, ref_mx = dbscan.dbscan_segment(ri, tm3, ground, 0.45, 10, brute_force=True, ws=arena.view)
    _clean(arena, "dbscan brute force")
    want = dbscan_ref.dbscan_frame(ris[0], inp["tm_np"], gms[0], 0.45, 10)
    assert np.array_equal(ref_seg[0].cpu().numpy(), want) and int(ref_mx[0]) == want.max() and want.max() >= 4
    for pattern in SIDE_PATTERNS:
        arena.fill(pattern)
        seg, mx = dbscan.dbscan_segment(ri, tm3, ground, 0.45, 10, ws=arena.view)
        assert torch.equal(seg, ref_seg) and torch.equal(mx, ref_mx), pattern
        _clean(arena, "dbscan, workspace %s" % pattern)


def test_eval_workspace(env):
    """rpcc_eval_nn / _normals / _metrics on rpcc_eval_workspace_bytes, one workspace for the three as quality_batch uses it: nearest neighbours
    and the D1 / D2 sums against tests/eval_ref.py, normals against the run on a zeroed workspace (which test_gpu_eval_metrics holds to numpy).
    Two deliberate exceptions to "bit for bit against the reference": the D1 / D2 means are float64 sums whose order differs between the device
    and numpy, so they are held to eval_ref within 1e-9 relative, the bound test_gpu_eval_metrics::test_d1_d2_against_numpy sets; and the
    normals have no comparison with eval_ref here.  What this test is about -- that the workspace's contents do not matter -- has no
    tolerance: every pattern's distances, indices, normals and sums equal the zero-workspace run's bit for bit."""
    torch, ops = env["torch"], env["ops"]
    import eval_ref as R
    from rpcc_amd import _eval_lib, evaluate_metrics as em
    inp = _inputs(env, "16x1800", "default")
    g = inp["g"]
    ris, _ = BC.grounds("16x1800", "default")
    rng = np.random.default_rng(5)
    a = np.stack([ris[0], ris[1]])
    b = (a + (a != 0) * rng.uniform(-0.02, 0.02, a.shape)).astype(np.float32)
    b[0, 3, 100:140] = 0                                           # the clouds differ in size
    tm3 = inp["tm"].reshape(g.H, g.W, 3)
    p1, p2 = ops.backproject(_to(env, a), tm3), ops.backproject(_to(env, b), tm3)
    arena = Arena(int(_eval_lib.lib().rpcc_eval_workspace_bytes(2, g.H, g.W)), env["dev"])
    ref = None
    for pattern in ("zero",) + SIDE_PATTERNS[1:]:
        arena.fill(pattern)
        d1, i1, d2, i2, n, _ = em.nearest(p1, p2, ws=arena.view)
        _clean(arena, "eval_nn, workspace %s" % pattern)
        arena.fill(pattern)
        nrm, _ = em.normals(p1, ws=arena.view)
        _clean(arena, "eval_normals, workspace %s" % pattern)
        arena.fill(pattern)
        sums = em.frame_sums(p1, p2, i1, i2, nrm, ws=arena.view)
        _clean(arena, "eval_metrics, workspace %s" % pattern)
        nn = n.cpu().numpy()
        got = [t.cpu().numpy() for t in (d1, i1, d2, i2, nrm, sums)]
        if ref is None:
            ref = got
            for f in range(2):
                c1, c2 = R.compact(p1[f].cpu().numpy()), R.compact(p2[f].cpu().numpy())
                assert (nn[f, 0], nn[f, 1]) == (c1.shape[0], c2.shape[0])
                qs = np.sort(rng.choice(c1.shape[0], 2000, replace=False))
                rd, ri_ = R.nn(c1[qs], c2, hint=got[1][f, :nn[f, 0]][qs])
                assert np.array_equal(got[0][f, :nn[f, 0]][qs].view(np.uint32), rd.astype(np.float32).view(np.uint32)) and np.array_equal(got[1][f, :nn[f, 0]][qs], ri_)
                w = R.d1_d2(c1, c2, got[1][f, :nn[f, 0]].astype(np.int64), got[3][f, :nn[f, 1]].astype(np.int64), got[4][f, :nn[f, 0]])
                s = got[5][f]
                mse = (s[4] / s[0], s[5] / s[1], s[8] / s[0], s[9] / s[1])
                for x, y in zip(mse, w):
                    assert abs(x - y) <= 1e-9 * abs(y), (f, mse, w)
            continue
        for f in range(2):
            for k in (0, 1, 4):
                assert _beq(got[k][f, :nn[f, 0]], ref[k][f, :nn[f, 0]]), (pattern, f, k)
            for k in (2, 3):
                assert _beq(got[k][f, :nn[f, 1]], ref[k][f, :nn[f, 1]]), (pattern, f, k)
        assert _beq(got[5], ref[5]), pattern


def _side_sources():
    """Three of the entropy coders' edge inputs and one golden array."""
    import deflate_cases
    rng = np.random.default_rng(7)
    far = np.zeros(70000, np.uint8)
    far[100:120] = rng.integers(1, 256, 20, dtype=np.uint8)
    far[65535 + 100: 65535 + 120] = far[100:120]
    gold = deflate_cases.golden_arrays()
    k = sorted(gold)[0]
    return {"len13": rng.integers(0, 4, 13, dtype=np.uint8).tobytes(), "len65537": rng.integers(0, 4, 65537, dtype=np.uint8).tobytes(),
            "offset_65535": far.tobytes(), "golden_" + k: bytes(gold[k])}


def _descriptors(env, srcs):
    torch = env["torch"]
    data = [torch.frombuffer(bytearray(s), dtype=torch.uint8).to(env["dev"]) for s in srcs]
    desc = torch.tensor([[t.data_ptr() for t in data], [len(s) for s in srcs]], dtype=torch.int64, device=env["dev"])
    return data, desc


def test_lz4_buffers(env):
    """rpcc_lz4_encode / rpcc_lz4_decode write into slots of the caller's buffer and rpcc_lz4_pack_containers takes a work buffer: each an arena
    of the exact size under every pattern; streams equal tests/lz4_ref.py, what lies between and behind the streams is left as it was."""
    torch = env["torch"]
    import lz4_ref
    from rpcc_amd import _lz4_lib as L, lz4_codec
    from rpcc_amd._lib import ptr, stream
    src = _side_sources()
    srcs = list(src.values())
    n = len(srcs)
    want = [lz4_ref.dumps(s) for s in srcs]
    data, desc = _descriptors(env, srcs)
    cap = np.array([lz4_codec.bound(len(s)) for s in srcs], np.int64)
    off = np.zeros(n, np.int64)                       # slots at 8-byte aligned offsets, as lz4_codec lays them out for the decoder's input
    off[1:] = np.cumsum((cap + 7) // 8 * 8)[:-1]
    meta = _to(env, np.stack([off, cap]))
    enc = Arena(int(off[-1] + cap[-1]), env["dev"])   # (the last slot ends the buffer: no slack behind it)
    dcap = np.array([len(s) for s in srcs], np.int64)
    doff = np.zeros(n, np.int64)
    doff[1:] = np.cumsum((dcap + 7) // 8 * 8)[:-1]
    dmeta = _to(env, np.stack([doff, dcap]))
    dec = Arena(int(doff[-1] + dcap[-1]), env["dev"])
    ws = Arena(max(int(L.lib().rpcc_lz4_workspace_bytes(n)), 8), env["dev"])
    for pattern in SIDE_PATTERNS:
        enc.fill(pattern), dec.fill(pattern), ws.fill(pattern)
        before, dbefore = enc.view.clone(), dec.view.cpu().numpy().copy()
        dst_len = filled((n,), torch.int64, env["dev"], POISON)
        L.check(L.lib().rpcc_lz4_encode(ptr(desc[0]), ptr(desc[1]), n, ptr(enc.view), ptr(meta[0]), ptr(meta[1]), ptr(dst_len), stream()))
        got = dst_len.cpu().numpy()
        h = enc.view.cpu().numpy()
        keep = np.ones(h.size, bool)
        for k in range(n):
            assert h[off[k]: off[k] + got[k]].tobytes() == want[k], (pattern, list(src)[k])
            keep[off[k]: off[k] + got[k]] = False
        assert np.array_equal(h[keep], before.cpu().numpy()[keep]), pattern          # the slots' unused ends
        _clean(enc, "lz4_encode, %s" % pattern)
        # the decoder on those streams, in place in the encoder's arena
        sdesc = torch.tensor([[enc.view.data_ptr() + int(o) for o in off], got.tolist()], dtype=torch.int64, device=env["dev"])
        out_len = filled((n,), torch.int64, env["dev"], POISON)
        status = filled((n,), torch.int32, env["dev"], POISON)
        L.check(L.lib().rpcc_lz4_decode(ptr(sdesc[0]), ptr(sdesc[1]), n, ptr(dec.view), ptr(dmeta[0]), ptr(dmeta[1]), ptr(out_len), ptr(status), stream()))
        assert not status.cpu().numpy().any() and np.array_equal(out_len.cpu().numpy(), dcap), pattern
        hd, dkeep = dec.view.cpu().numpy(), np.ones(dec.nbytes, bool)
        for k in range(n):
            assert hd[doff[k]: doff[k] + dcap[k]].tobytes() == srcs[k], (pattern, list(src)[k])
            dkeep[doff[k]: doff[k] + dcap[k]] = False
        assert np.array_equal(hd[dkeep], dbefore[dkeep]), pattern                      # the gaps between the outputs
        _clean(dec, "lz4_decode, %s" % pattern)
        # containers: two frames of two streams
        out, frame = lz4_codec.pack_containers(enc.view, meta[0], dst_len, 2, 2, int(got.sum()) + 4 * n, ws=ws.view)
        fr = frame.cpu().numpy()
        o = out.cpu().numpy()
        for f in range(2):
            blob = o[fr[0, f]: fr[0, f] + fr[1, f]].tobytes()
            assert blob == b"".join(len(want[2 * f + k]).to_bytes(4, "little") + want[2 * f + k] for k in range(2)), (pattern, f)
        _clean(ws, "lz4_pack_containers, %s" % pattern)


def test_deflate_workspace(env):
    """rpcc_deflate_encode on rpcc_deflate_workspace_bytes(n, total) bytes: the streams of tests/deflate_ref.py under every pattern."""
    torch = env["torch"]
    import deflate_ref
    from rpcc_amd import _deflate_lib as L, deflate_codec
    src = _side_sources()
    srcs = list(src.values())
    n = len(srcs)
    want = [deflate_ref.compress(s) for s in srcs]
    data, desc = _descriptors(env, srcs)
    sizes = [len(s) for s in srcs]
    ws = Arena(int(L.lib().rpcc_deflate_workspace_bytes(n, sum(sizes))), env["dev"])
    for pattern in SIDE_PATTERNS:
        ws.fill(pattern)
        slots, _, dst_len, off = deflate_codec.encode_descriptors(desc[0], desc[1], sizes, ws=ws.view)
        got, h = dst_len.cpu().numpy(), slots.cpu().numpy()
        for k in range(n):
            assert h[off[k]: off[k] + got[k]].tobytes() == want[k], (pattern, list(src)[k])
        _clean(ws, "deflate_encode, workspace %s" % pattern)


# ------------------------------------------------------------------------------------------------
# f. every output byte is accounted for
# ------------------------------------------------------------------------------------------------
def _report(holes, allowed, tag):
    """holes / allowed: {name: bool over bytes}.  The sets must be equal; the message names what differs."""
    msgs = []
    for k in holes:
        h = holes[k].cpu().numpy()
        a = np.zeros(h.shape, bool) if allowed.get(k) is None else np.asarray(allowed[k]).reshape(-1)
        extra, missing = np.flatnonzero(h & ~a), np.flatnonzero(~h & a)
        if extra.size:
            msgs.append("%s: %d of %d bytes left unwritten that the header does not list (byte offsets %d .. %d)" % (k, extra.size, h.size, extra[0], extra[-1]))
        if missing.size:
            msgs.append("%s: %d bytes written (or not repeatable) that the header lists as left alone (byte offsets %d .. %d)" % (k, missing.size, missing[0], missing[-1]))
    assert not msgs, (tag, msgs)


def _tail(n_rows, width, starts, itemsize):
    """bool [n_rows * width * itemsize]: the bytes of elements [starts[b]:] of every row."""
    m = np.arange(width)[None, :] >= np.asarray(starts).reshape(-1, 1)
    return np.repeat(m.reshape(-1), itemsize)


@pytest.mark.parametrize("M,variant", [(100, "uniform_point"), (100, "nonuniform_plane"), (300, "uniform_point"), (300, "nonuniform_plane")])
def test_fused_batch_unwritten_bytes(env, M, variant):
    """The fused call at 5 x 300, byte and uint16 labels, both frameworks: the output bytes it leaves alone are exactly those the header lists --
    q16 past nnz, and salience / key_point_map in the uniform framework (they are not even handed in) -- and everything else repeats bit for bit."""
    ops = env["ops"]
    inp = _inputs(env, "5x300", "default")
    arena = Arena(_ws_bytes(env, inp, M, variant), env["dev"])
    kw = _kw(env, M, variant)

    def run(fill_byte):
        arena.fill("alt(0,%d)" % (fill_byte & 1))
        buf = _buffers(env, inp, M, variant, arena.view)
        _poison(buf, fill_byte)
        gfit = filled((inp["B"], 4), env["torch"].float64, env["dev"], fill_byte)
        ops.compress_batch(inp["xyz"], inp["offs"], inp["tm"], gfit, buf, **kw)
        env["torch"].cuda.synchronize()
        out = {f: getattr(buf, f) for f in OUTPUTS}
        out["ground"] = gfit
        return out

    outs = {}
    holes = unwritten(run, outs)
    nnz = outs["nnz"].cpu().numpy()
    allowed = {"q16": _tail(inp["B"], inp["P"], nnz, 2)}
    if variant == "uniform_point":
        allowed["salience"] = np.ones(holes["salience"].numel(), bool)
        allowed["key_point_map"] = np.ones(holes["key_point_map"].numel(), bool)
    _report(holes, allowed, ("fused", M, variant))
    _clean(arena, "fused unwritten")


@pytest.mark.parametrize("name,M", [("5x300", 100), ("16x1800", 300)])
def test_stage_entries_unwritten_bytes(env, name, M):
    """The stage entries of (d): projection, mask + FPS, point model, plane model, quantiser (q16 past nnz is left alone: predict_quantize needs no
    zero-filled q), rpcc_pack_payload (packed past total is left alone), contour codec (idx_sequence past nseq is left alone), decoder (pc_rec is written when given)."""
    ops, torch, dev = env["ops"], env["torch"], env["dev"]
    s = _stage_inputs(env, name, M)
    inp = s["inp"]
    g, B, P, K = inp["g"], inp["B"], inp["P"], M + 2
    lab = torch.uint16 if M > 254 else torch.uint8
    lib = env["lib"]

    def project(fb):
        return dict(ri=ops.project(inp["xyz"], inp["offs"], inp["geom"], ri=filled((B, g.H, g.W), torch.float32, dev, fb)))
    _report(unwritten(project), {}, (name, "project"))

    # the remaining entries allocate their outputs themselves (torch.empty): pre-fill through the caching allocator is not possible, so they are
    # called through the C ABI with filled buffers
    from rpcc_amd._lib import check, ptr, stream
    L = lib.lib()
    wide = M > 254

    def mask_fps(fb):
        temp, info = filled((B, P), torch.float32, dev, fb), filled((B, lib.INFO_INTS), torch.int32, dev, fb)
        tab = filled((int(L.rpcc_fps_table_bytes(B, g.H, g.W)),), torch.uint8, dev, fb)
        check(L.rpcc_ground_mask(ptr(s["ri"]), ptr(inp["tm"]), ptr(s["ground"]), BC.GROUND_THRESHOLD, B, g.H, g.W, ptr(temp), ptr(info), ptr(tab), stream()))
        cen, ctr = filled((B, M), torch.int32, dev, fb), filled((B, M, 3), torch.float32, dev, fb)
        check(L.rpcc_fps_range(ptr(s["ri"]), ptr(inp["tm"]), ptr(temp), ptr(info), B, g.H, g.W, M, ptr(cen), ptr(ctr), 0, ptr(tab), stream()))
        return dict(temp=temp, info=info, cen_pix=cen, centers=ctr)
    _report(unwritten(mask_fps), {}, (name, "ground_mask + fps_range"))

    ws = torch.empty(int(L.rpcc_workspace_bytes(B, P, M, 0)), dtype=torch.uint8, device=dev)

    def point_model(fb):
        model, counts = filled((B, K, 4), torch.float32, dev, fb), filled((B, K), torch.int32, dev, fb)
        check((L.rpcc_point_model_wide if wide else L.rpcc_point_model)(ptr(s["ri"]), ptr(s["seg"]), ptr(s["ground"]), B, P, M, ptr(model), ptr(counts), ptr(ws), stream()))
        return dict(model=model, counts=counts)
    _report(unwritten(point_model), {}, (name, "point_model"))

    pws = torch.empty(int(L.rpcc_plane_workspace_bytes(B, P, M)), dtype=torch.uint8, device=dev)

    def plane_model(fb):
        model, counts = filled((B, K, 4), torch.float32, dev, fb), filled((B, K), torch.int32, dev, fb)
        check((L.rpcc_plane_model_wide if wide else L.rpcc_plane_model)(ptr(s["ri"]), ptr(inp["tm"]), ptr(s["seg"]), ptr(s["ground"]), B, P, M, ops.angle_cos_cut(BC.ANGLE),
                                                                        BC.PLANE_SEED, None, None, ptr(model), ptr(counts), ptr(pws), stream()))
        return dict(model=model, counts=counts)
    _report(unwritten(plane_model), {}, (name, "plane_model"))

    def quantise(fb):
        q16, q32 = filled((B, P), torch.int16, dev, fb), filled((B, P), torch.int32, dev, fb)
        nnz, pred = filled((B,), torch.int32, dev, fb), filled((B, P), torch.float32, dev, fb)
        fn = L.rpcc_predict_quantize_wide if wide else L.rpcc_predict_quantize
        check(fn(ptr(s["ri"]), ptr(inp["tm"]), ptr(s["seg"]), ptr(s["model_u"]), None, None, BC.ACC, B, P, M, ptr(q16), ptr(q32), ptr(nnz), ptr(pred), ptr(ws), stream()))
        return dict(q16=q16, q32=q32, nnz=nnz, pred=pred)
    outs = {}
    holes = unwritten(quantise, outs)
    nnz = outs["nnz"].cpu().numpy()
    _report(holes, {"q16": _tail(B, P, nnz, 2), "q32": _tail(B, P, nnz, 4)}, (name, "predict_quantize"))
    q16, d_nnz = outs["q16"], outs["nnz"]

    def pack(fb):
        packed, total = filled((B * P,), torch.int16, dev, fb), filled((1,), torch.int64, dev, fb)
        check(L.rpcc_pack_payload(ptr(q16), ptr(d_nnz), B, P, ptr(packed), B * P, ptr(total), stream()))
        return dict(packed=packed, total=total)
    outs = {}
    holes = unwritten(pack, outs)
    assert int(outs["total"]) == int(nnz.sum()) > 0
    _report(holes, {"packed": _tail(1, B * P, [int(nnz.sum())], 2)}, (name, "pack_payload"))

    cws = torch.empty(_codec_bytes(env, inp, M), dtype=torch.uint8, device=dev)

    def encode(fb):
        bits, seq, nseq = filled((B, (P + 7) // 8), torch.uint8, dev, fb), filled((B, P), torch.uint16, dev, fb), filled((B,), torch.int32, dev, fb)
        check((L.rpcc_contour_encode_wide if wide else L.rpcc_contour_encode)(ptr(s["seg"]), B, g.H, g.W, ptr(bits), ptr(seq), ptr(nseq), ptr(cws), stream()))
        return dict(contour_bits=bits, idx_sequence=seq, nseq=nseq)
    outs = {}
    holes = unwritten(encode, outs)
    _report(holes, {"idx_sequence": _tail(B, P, outs["nseq"].cpu().numpy(), 2)}, (name, "contour_encode"))
    bits, seq = outs["contour_bits"], outs["idx_sequence"]

    def decode(fb):
        seg = filled((B, g.H, g.W), lab, dev, fb)
        check((L.rpcc_contour_decode_wide if wide else L.rpcc_contour_decode)(ptr(bits), ptr(seq), B, g.H, g.W, ptr(seg), ptr(cws), stream()))
        rec, pc = filled((B, P), torch.float32, dev, fb), filled((B, P, 3), torch.float32, dev, fb)
        acc = (C.c_double * 1)(BC.ACC)
        q16 = torch.zeros((B, P), dtype=torch.int16, device=dev)
        check((L.rpcc_decode_wide if wide else L.rpcc_decode)(ptr(seg), ptr(q16), ptr(s["model_u"]), ptr(inp["tm"]), acc, 0, None, B, P, M, ptr(rec), ptr(pc), ptr(cws), stream()))
        return dict(seg=seg, ri_rec=rec, pc_rec=pc)
    _report(unwritten(decode), {}, (name, "contour_decode + decode"))


def test_side_libraries_unwritten_bytes(env):
    """rpcc_seg_dbscan writes every label and maximum, and its stats -- work counters that depend on the order in which a workgroup's lanes
    list the tiles, so they are written (never the fill) but need not repeat; rpcc_eval_nn leaves the entries past each cloud's point count
    alone (n says how many are valid), rpcc_eval_normals the rows past it; rpcc_eval_metrics writes all ten sums."""
    torch, ops, dev = env["torch"], env["ops"], env["dev"]
    from rpcc_amd import _eval_lib as E, _seg_lib as S
    from rpcc_amd._lib import ptr, stream
    inp = _inputs(env, "16x1800", "default")
    g = inp["g"]
    H, W, P = g.H, g.W, inp["P"]
    ris, gms = BC.grounds("16x1800", "default")
    ri = _to(env, np.stack([ris[0], ris[1]]))
    ground = _to(env, np.stack([gms[0], gms[1]]))
    tm3 = inp["tm"].reshape(H, W, 3)
    sws = torch.empty(int(S.lib().rpcc_seg_workspace_bytes(2, H, W)), dtype=torch.uint8, device=dev)

    def seg(fb):
        out, mx, st = filled((2, H, W), torch.int32, dev, fb), filled((2,), torch.int32, dev, fb), filled((2, S.NSTATS), torch.int64, dev, fb)
        S.check(S.lib().rpcc_seg_dbscan(ptr(ri), ptr(tm3), ptr(ground), 2, H, W, 0.45, 10, 0, ptr(out), ptr(mx), ptr(st), ptr(sws), stream()))
        stats[fb] = st.cpu().numpy()
        return dict(seg=out, max_label=mx)
    stats = {}
    _report(unwritten(seg), {}, "seg_dbscan")
    for fb, st in stats.items():      # written in both runs: counts, not the fill (0xFF bytes read as -1)
        assert (st > 0).all() and (st < 1 << 40).all(), (fb, st)

    p1 = ops.backproject(ri, tm3)
    p2 = ops.backproject((ri * 1.001).contiguous(), tm3)
    ews = torch.empty(int(E.lib().rpcc_eval_workspace_bytes(2, H, W)), dtype=torch.uint8, device=dev)

    def nn(fb):
        d1, d2 = filled((2, P), torch.float32, dev, fb), filled((2, P), torch.float32, dev, fb)
        i1, i2 = filled((2, P), torch.int32, dev, fb), filled((2, P), torch.int32, dev, fb)
        n = filled((2, 2), torch.int32, dev, fb)
        E.check(E.lib().rpcc_eval_nn(ptr(p1), ptr(p2), 2, H, W, 0, ptr(d1), ptr(i1), ptr(d2), ptr(i2), ptr(n), None, ptr(ews), stream()))
        return dict(dist1=d1, idx1=i1, dist2=d2, idx2=i2, n=n)
    outs = {}
    holes = unwritten(nn, outs)
    n = outs["n"].cpu().numpy()
    _report(holes, {"dist1": _tail(2, P, n[:, 0], 4), "idx1": _tail(2, P, n[:, 0], 4), "dist2": _tail(2, P, n[:, 1], 4), "idx2": _tail(2, P, n[:, 1], 4)}, "eval_nn")

    def metrics(fb):
        nrm = filled((2, P, 3), torch.float64, dev, fb)
        E.check(E.lib().rpcc_eval_normals(ptr(p1), 2, H, W, 59.7, 0, ptr(nrm), None, ptr(ews), stream()))
        sums = filled((2, E.NSUMS), torch.float64, dev, fb)
        E.check(E.lib().rpcc_eval_metrics(ptr(p1), ptr(p2), 2, H, W, ptr(outs["idx1"]), ptr(outs["idx2"]), ptr(nrm), float(np.float32(0.02 ** 2)), ptr(sums), ptr(ews), stream()))
        return dict(normals=nrm, sums=sums)
    holes = unwritten(metrics)
    _report(holes, {"normals": _tail(2, P, n[:, 0], 24)}, "eval_normals + eval_metrics")


def _members(nbytes, off, lens):
    """bool [nbytes]: True outside the byte ranges [off[k], off[k] + lens[k]) of the entries with lens[k] > 0."""
    m = np.ones(nbytes, bool)
    for o, n in zip(off, lens):
        if n > 0:
            m[o: o + n] = False
    return m


def test_entropy_coders_unwritten_bytes(env):
    """rpcc_deflate_encode, rpcc_lz4_encode, rpcc_lz4_decode and rpcc_lz4_pack_containers through the C ABI on pre-filled outputs, six streams
    in slots with gaps between them, the last slot too small (a refused stream; with it the third container fails).  As the headers say: dst is
    written only where a member / stream lands -- the rest of a slot, the gaps and the refused stream's slot are left alone --, out only where a
    container lands, and dst_len, status, frame_off, frame_len are written for every stream / frame."""
    torch, dev = env["torch"], env["dev"]
    from rpcc_amd import _deflate_lib as D, _lz4_lib as L, deflate_codec, lz4_codec
    from rpcc_amd._lib import ptr, stream
    srcs = list(_side_sources().values())
    srcs += [srcs[1], srcs[0]]
    n, refused = len(srcs), len(srcs) - 1
    sizes = [len(s) for s in srcs]
    data, desc = _descriptors(env, srcs)

    def layout(bound):
        cap = np.array([bound(z) for z in sizes], np.int64)
        cap[refused] = 8
        off = np.zeros(n, np.int64)
        off[1:] = np.cumsum((cap + 7) // 8 * 8 + 8)[:-1]          # 8 .. 15 bytes between a slot's end and the next slot
        return off, _to(env, np.stack([off, cap])), int(off[-1] + cap[-1]) + 8

    off, meta, nb = layout(deflate_codec.bound)
    dws = torch.empty(int(D.lib().rpcc_deflate_workspace_bytes(n, sum(sizes))), dtype=torch.uint8, device=dev)

    def deflate(fb):
        dst, dst_len = filled((nb,), torch.uint8, dev, fb), filled((n,), torch.int64, dev, fb)
        D.check(D.lib().rpcc_deflate_encode(ptr(desc[0]), ptr(desc[1]), n, sum(sizes), ptr(dst), ptr(meta[0]), ptr(meta[1]), ptr(dst_len), ptr(dws), stream()))
        return dict(dst=dst, dst_len=dst_len)
    outs = {}
    holes = unwritten(deflate, outs)
    lens = outs["dst_len"].cpu().numpy()
    assert lens[refused] == D.E_CAPACITY and (lens[:refused] > 0).all(), lens
    _report(holes, {"dst": _members(nb, off, lens)}, "deflate_encode")

    off, meta, nb = layout(lz4_codec.bound)

    def encode(fb):
        dst, dst_len = filled((nb,), torch.uint8, dev, fb), filled((n,), torch.int64, dev, fb)
        L.check(L.lib().rpcc_lz4_encode(ptr(desc[0]), ptr(desc[1]), n, ptr(dst), ptr(meta[0]), ptr(meta[1]), ptr(dst_len), stream()))
        return dict(dst=dst, dst_len=dst_len)
    outs = {}
    holes = unwritten(encode, outs)
    slots, d_len = outs["dst"], outs["dst_len"]
    lens = d_len.cpu().numpy()
    assert lens[refused] == L.E_CAPACITY and (lens[:refused] > 0).all(), lens
    _report(holes, {"dst": _members(nb, off, lens)}, "lz4_encode")

    # the decoder on the streams that were written
    m = refused
    sdesc = torch.tensor([[slots.data_ptr() + int(o) for o in off[:m]], lens[:m].tolist()], dtype=torch.int64, device=dev)
    dcap = np.array(sizes[:m], np.int64)
    doff = np.zeros(m, np.int64)
    doff[1:] = np.cumsum((dcap + 7) // 8 * 8 + 8)[:-1]
    dmeta = _to(env, np.stack([doff, dcap]))
    dn = int(doff[-1] + dcap[-1]) + 8

    def decode(fb):
        dst, out_len, status = filled((dn,), torch.uint8, dev, fb), filled((m,), torch.int64, dev, fb), filled((m,), torch.int32, dev, fb)
        L.check(L.lib().rpcc_lz4_decode(ptr(sdesc[0]), ptr(sdesc[1]), m, ptr(dst), ptr(dmeta[0]), ptr(dmeta[1]), ptr(out_len), ptr(status), stream()))
        return dict(dst=dst, dst_len=out_len, status=status)
    outs = {}
    holes = unwritten(decode, outs)
    assert not outs["status"].cpu().numpy().any() and np.array_equal(outs["dst_len"].cpu().numpy(), dcap)
    _report(holes, {"dst": _members(dn, doff, dcap)}, "lz4_decode")

    # three containers of two streams; the third holds the refused stream
    pws = torch.empty(max(int(L.lib().rpcc_lz4_workspace_bytes(n)), 8), dtype=torch.uint8, device=dev)
    good = int(lens[:4].sum()) + 4 * 4
    out_cap = good + 64

    def pack(fb):
        out, fo, fl = filled((out_cap,), torch.uint8, dev, fb), filled((3,), torch.int64, dev, fb), filled((3,), torch.int64, dev, fb)
        L.check(L.lib().rpcc_lz4_pack_containers(ptr(slots), ptr(meta[0]), ptr(d_len), 3, 2, ptr(out), out_cap, ptr(fo), ptr(fl), ptr(pws), stream()))
        return dict(out=out, frame_off=fo, frame_len=fl)
    outs = {}
    holes = unwritten(pack, outs)
    fo, fl = outs["frame_off"].cpu().numpy(), outs["frame_len"].cpu().numpy()
    assert fl[2] == -1 and fl[0] + fl[1] == good, (fo, fl)
    _report(holes, {"out": _members(out_cap, fo, fl)}, "lz4_pack_containers")


# ------------------------------------------------------------------------------------------------
# the alignment the headers state
# ------------------------------------------------------------------------------------------------
def _at_alignment(env, nbytes, shift, f, what):
    """f(work buffer) -> tensors, on a 256-byte aligned buffer and on one at base + shift, both of exactly nbytes bytes under half(1): the same bytes
    out, nothing written in front of or behind the shifted buffer."""
    torch = env["torch"]
    ref = f(Arena(nbytes, env["dev"]).fill("half(1)").view)
    a = Arena(nbytes + shift, env["dev"]).fill("half(1)")
    head = a.view[:shift].clone()
    ws = a.view[shift:]
    assert ws.data_ptr() % 256 == shift and ws.numel() == nbytes
    got = f(ws)
    for k, (x, y) in enumerate(zip(ref, got)):
        assert torch.equal(x.contiguous().reshape(-1).view(torch.uint8), y.contiguous().reshape(-1).view(torch.uint8)), (what, k)
    assert torch.equal(a.view[:shift], head), (what, "bytes in front of the buffer were written")
    _clean(a, what)


def test_work_buffers_at_the_stated_alignment(env):
    """The headers ask for less than the 256 bytes every other test uses: 16 bytes for librpcc_hip, seg and eval, 8 for lz4 and deflate.  One
    call of every kind of work buffer at exactly that alignment (5 x 300, M = 100 and 300; the side libraries' cases of (e))."""
    torch, ops, dev = env["torch"], env["ops"], env["dev"]
    lib = env["lib"].lib()
    inp = _inputs(env, "5x300", "default")
    B, P, g = inp["B"], inp["P"], inp["g"]
    for M in (100, 300):
        for variant in BC.VARIANTS:
            exp = BC.expected("5x300", M, variant)
            for pattern in ("alt(0,1)", "half(0)"):
                a = Arena(_ws_bytes(env, inp, M, variant) + 16, dev).fill(pattern)
                head = a.view[:16].clone()
                buf = _buffers(env, inp, M, variant, a.view[16:])
                gfit = _ground_out(env, B)
                ops.compress_batch(inp["xyz"], inp["offs"], inp["tm"], gfit, buf, **_kw(env, M, variant))
                _check(env, inp, buf, gfit, exp, M, variant, ("base + 16", M, variant, pattern))
                assert buf.ws.data_ptr() == a.view.data_ptr() + 16 and torch.equal(a.view[:16], head)
                _clean(a, "compress_batch at base + 16, M=%d %s %s" % (M, variant, pattern))
        s = _stage_inputs(env, "5x300", M)
        _at_alignment(env, int(lib.rpcc_workspace_bytes(B, P, M, 0)), 16, lambda ws: ops.point_model(s["ri"], s["seg"], s["ground"], M, ws=ws), "point_model")
        _at_alignment(env, int(lib.rpcc_workspace_bytes(B, P, M, 0)), 16,
                      lambda ws: ops.predict_quantize(s["ri"], inp["tm"], s["seg"], s["model_u"], BC.ACC, M, want_pred=True, int16=True, ws=ws), "predict_quantize")
        _at_alignment(env, int(lib.rpcc_plane_workspace_bytes(B, P, M)), 16,
                      lambda ws: ops.plane_model(s["ri"], inp["tm"], s["seg"], M, angle_threshold=BC.ANGLE, seed=BC.PLANE_SEED, ground=s["ground"], want_counts=True, ws=ws),
                      "plane_model")

        def codec(ws):
            bits, seq, nseq = ops.contour_encode(s["seg"], M, ws=ws)
            seg_rec = ops.contour_decode(bits, seq, g.H, g.W, M, ws=ws)
            rec, pc = ops.decode(seg_rec, torch.zeros((B, P), dtype=torch.int16, device=dev), s["model_u"], inp["tm"], BC.ACC, want_points=True, ws=ws)
            return bits, nseq, seg_rec, rec, pc
        _at_alignment(env, _codec_bytes(env, inp, M), 16, codec, "contour codec and decoder")
    _at_alignment(env, int(lib.rpcc_project_scratch_bytes(inp["total"], B, P)), 16, lambda ws: (ops.project(inp["xyz"], inp["offs"], inp["geom"], scratch=ws),), "project")
    _at_alignment(env, B * (P + 8) * 4, 16, lambda ws: (ops.project(inp["xyz"], inp["offs"], inp["geom"], scratch=ws, atomic_path=True),), "project, atomic path")
    s = _stage_inputs(env, "5x300", 100)

    def fps(ws):
        temp, info, tab = ops.ground_mask(s["ri"], inp["tm"], s["ground"], BC.GROUND_THRESHOLD, fps_table=True, table=ws)
        return (temp, info) + tuple(ops.fps_range(s["ri"], inp["tm"], temp, info, 100, fps_table=tab))
    _at_alignment(env, int(lib.rpcc_fps_table_bytes(B, g.H, g.W)), 16, fps, "fps table")

    # the side libraries
    from rpcc_amd import _deflate_lib, _eval_lib, _lz4_lib, _seg_lib, dbscan, deflate_codec, evaluate_metrics as em, lz4_codec
    big = _inputs(env, "16x1800", "default")
    H, W = big["g"].H, big["g"].W
    ris, gms = BC.grounds("16x1800", "default")
    ri, ground = _to(env, np.stack([ris[0], ris[1]])), _to(env, np.stack([gms[0], gms[1]]))
    tm3 = big["tm"].reshape(H, W, 3)
    _at_alignment(env, int(_seg_lib.lib().rpcc_seg_workspace_bytes(2, H, W)), 16, lambda ws: dbscan.dbscan_segment(ri, tm3, ground, 0.45, 10, ws=ws), "dbscan")
    p1, p2 = ops.backproject(ri, tm3), ops.backproject((ri * 1.001).contiguous(), tm3)

    def metrics(ws):
        _, i1, _, i2, n, _ = em.nearest(p1, p2, ws=ws)
        nrm, _ = em.normals(p1, ws=ws)
        return n, em.frame_sums(p1, p2, i1, i2, nrm, ws=ws)
    _at_alignment(env, int(_eval_lib.lib().rpcc_eval_workspace_bytes(2, H, W)), 16, metrics, "eval")

    srcs = list(_side_sources().values())
    sizes = [len(x) for x in srcs]
    data, desc = _descriptors(env, srcs)

    def deflate(ws):
        slots, _, dst_len, off = deflate_codec.encode_descriptors(desc[0], desc[1], sizes, ws=ws)
        return (dst_len,) + tuple(slots[o: o + n] for o, n in zip(off.tolist(), dst_len.tolist()))
    _at_alignment(env, int(_deflate_lib.lib().rpcc_deflate_workspace_bytes(len(srcs), sum(sizes))), 8, deflate, "deflate_encode")
    slots, d_off, d_len, _ = lz4_codec.encode_descriptors(desc[0], desc[1], sizes)
    total = int(d_len.sum()) + 4 * len(srcs)

    def pack(ws):
        out, frame = lz4_codec.pack_containers(slots, d_off, d_len, 2, 2, total, ws=ws)
        return frame, out[:total]
    _at_alignment(env, max(int(_lz4_lib.lib().rpcc_lz4_workspace_bytes(len(srcs))), 8), 8, pack, "lz4_pack_containers")
