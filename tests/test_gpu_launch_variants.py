"""-m gpu: every kernel variant the launch code of librpcc_hip can pick (tests/launch_variants.py: the rules restated, the case tables),
at the smallest shapes that reach it, bit for bit against the CPU oracle.

FPS: the fused entry, the stage entries and the list entry at the frame counts, tile counts and widths that select each instantiation
(1024 / 512 threads; planar, planar2, register table, LDS table; 16-byte, EDGE and element-wise accesses), the one-pass kernel past
3200 tiles, one mixed call of 130 frames.  Data arrays at their natural alignment (a view one element into a larger tensor) against the
same arrays 256-byte aligned.  The six chunk-length classes of the key-point kernel at both widths per wavefront and on both label
types, with their boundaries.  The assignment at the cluster counts where its label type and its screening rounds change.

A batch of 129 frames holds at most five distinct scenes in rotation (frame_ids = scene number, so the seeded ground fit is per scene):
the oracle runs once per scene and every frame is compared."""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import launch_variants as lv

pytestmark = pytest.mark.gpu
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


def _beq(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _np(t):
    return t.cpu().numpy()


@functools.lru_cache(maxsize=4)
def _shape(H, W):
    """(oracle geometry, transform map) of an H x W image with the scenes' vertical field of view."""
    from oracle import oracle as orc
    g = lv.geom_of(H, W)
    return g, orc.transform_map(g)


def _geom(env, H, W):
    g, tm = _shape(H, W)
    ops = env["ops"]
    assert np.array_equal(ops.transform_map(g.H, g.W, g.horizontal_FOV, g.vertical_max, g.vertical_min), tm)
    return g, ops.make_geom(g.H, g.W, g.horizontal_FOV, g.vertical_max, g.vertical_min), tm


@functools.lru_cache(maxsize=16)
def _oracle_scene(H, W, k, M):
    """The oracle on scene k of a shape: ground plane seeded with SEED + k (frame_ids = scene number), then the whole hot path.  One
    result per scene, shared by every test and every frame that shows the scene; nothing writes into it."""
    from oracle import oracle as orc
    g, tm = _shape(H, W)
    f = lv.scene_frame(H, W, k)
    ri = orc.project(f, g)
    gm = orc.ground_model(ri, tm, seed=SEED + k)
    o = orc.compress_frame(f, g, tm, gm, dict(orc.DEFAULT_CFG, cluster_num=M))
    assert len(set(o["fps_pix"].tolist())) == M, (H, W, k, "the scene must hold M distinct centres")
    return dict(ri=o["range_image"], gm=np.asarray(gm, np.float64), pix=o["fps_pix"], cen=o["centers"].astype(np.float32), seg=o["seg_idx"].astype(np.uint8),
                model=np.asarray(o["model_param"]).astype(np.float32), q=o["q"].astype(np.int16), mask=o["mask"])


def _oracle_scenes(H, W, n, M):
    with ThreadPoolExecutor(min(n, 16)) as ex:
        return list(ex.map(lambda k: _oracle_scene(H, W, k, M), range(n)))


def _batch(env, H, W, B):
    """B frames of an H x W image, the shape's scenes in rotation -> (xyz, offsets, frame ids on the device, scene number per frame)."""
    n = lv.n_scenes(H, W, B)
    scenes = [lv.scene_of(i, n) for i in range(B)]
    assert B == 1 or scenes[-1] != scenes[0]
    frames = [lv.scene_frame(H, W, k) for k in range(n)]
    offs = np.zeros(B + 1, np.int64)
    offs[1:] = np.cumsum([frames[k].shape[0] for k in scenes])
    return _to(env, np.concatenate([frames[k] for k in scenes])), _to(env, offs), _to(env, np.asarray(scenes, np.int64)), scenes


def _check_all(buf, gms, exp, scenes, tag):
    """Every output of every frame against the oracle's result of the frame's scene: range image, fitted ground plane, FPS pixels, centres,
    labels, model rows, quantised integers."""
    ri, seg, pix, cen = _np(buf.ri), _np(buf.seg), _np(buf.cen_pix), _np(buf.centers)
    gm, q, nz, mo = _np(gms), _np(buf.q16), _np(buf.nnz), _np(buf.model)
    for i, k in enumerate(scenes):
        o = exp[k]
        nrow = o["model"].shape[0]
        assert _beq(ri[i], o["ri"]), (tag, i, "range image")
        assert _beq(gm[i], o["gm"]), (tag, i, "ground plane")
        assert np.array_equal(pix[i], o["pix"]), (tag, i, "FPS pixels", pix[i], o["pix"])
        assert _beq(cen[i], o["cen"]), (tag, i, "centres")
        assert np.array_equal(seg[i].reshape(-1), o["seg"].reshape(-1)), (tag, i, "labels")
        assert _beq(mo[i, :nrow], o["model"]), (tag, i, "model rows")
        assert int(nz[i]) == o["q"].shape[0] and np.array_equal(q[i, :nz[i]], o["q"]), (tag, i, "quantised integers")


def _case_id(c):
    return "-".join(str(v) for v in c[:3]).replace(" ", "")


# ------------------------------------------------------------------------------------------------
# FPS: the fused entry
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,B,pick", lv.FPS_FUSED, ids=[_case_id(c) for c in lv.FPS_FUSED])
def test_fused_entry_fps_variants(env, H, W, B, pick):
    """rpcc_compress_batch at the shapes and frame counts of launch_variants.FPS_FUSED (the pick of each case is written there): every
    output of every frame equals the oracle's."""
    torch, ops = env["torch"], env["ops"]
    assert lv.fps_pick_range(H, W, B, 0, None, True) == pick
    M = lv.default_m(H, W)
    g, geom, tm = _geom(env, H, W)
    xyz, offs, fid, scenes = _batch(env, H, W, B)
    exp = _oracle_scenes(H, W, lv.n_scenes(H, W, B), M)
    buf = ops.BatchBuffers(B, geom, M, env["dev"], max_points=int(xyz.shape[0]))
    gms = torch.zeros((B, 4), dtype=torch.float64, device=env["dev"])
    d_tm = _to(env, tm)
    assert buf.ri.data_ptr() % 16 == 0 and d_tm.data_ptr() % 16 == 0          # the width alone decides the access form here
    ops.compress_batch(xyz, offs, d_tm, gms, buf, ground_seed=SEED, frame_ids=fid)
    torch.cuda.synchronize()
    _check_all(buf, gms, exp, scenes, (H, W, B) + pick)


@pytest.mark.parametrize("H,W,B", lv.FPS_FUSED_REFUSED)
def test_fused_entry_refuses_an_odd_image_past_the_tile_limit(env, H, W, B):
    """More than FPS_TILED_MAX_TILES tiles and a pixel count that is no multiple of four: the one-pass kernel reads 16 bytes at frame
    bases, so check_batch_io refuses the call with RPCC_ERR_ARG before anything is launched -- every output buffer stays as it was."""
    torch, ops = env["torch"], env["ops"]
    assert lv.fused_refuses(H, W, B)
    M = lv.default_m(H, W)
    g, geom, tm = _geom(env, H, W)
    xyz, offs, fid, scenes = _batch(env, H, W, B)
    buf = ops.BatchBuffers(B, geom, M, env["dev"], max_points=int(xyz.shape[0]))
    gms = torch.full((B, 4), 3.25, dtype=torch.float64, device=env["dev"])
    outs = ("ri", "seg", "cen_pix", "centers", "model", "counts", "q16", "nnz", "info")
    for f in outs:
        getattr(buf, f).view(torch.uint8).fill_(0xA5)
    with pytest.raises(env["lib"].RpccError, match=r"code -1"):
        ops.compress_batch(xyz, offs, _to(env, tm), gms, buf, ground_seed=SEED, frame_ids=fid)
    torch.cuda.synchronize()
    for f in outs:
        assert bool((getattr(buf, f).view(torch.uint8) == 0xA5).all()), f
    assert bool((gms == 3.25).all())


# ------------------------------------------------------------------------------------------------
# FPS: the stage entries (no planar ray table)
# ------------------------------------------------------------------------------------------------
def _stage_fps(env, ri, d_tm, gms, M, mode):
    ops = env["ops"]
    if mode == "tiled+table":
        temp, info, tab = ops.ground_mask(ri, d_tm, gms, 0.1, fps_table=True)
    else:
        (temp, info), tab = ops.ground_mask(ri, d_tm, gms, 0.1), None
    pix, cen = ops.fps_range(ri, d_tm, temp, info, M, fps_table=tab, bruteforce=(mode == "brute"))
    return _np(pix), _np(cen).view(np.uint32), _np(temp).view(np.uint32)


@pytest.mark.parametrize("H,W,B,pick", lv.FPS_STAGE, ids=[_case_id(c) for c in lv.FPS_STAGE])
def test_stage_entries_fps_variants(env, H, W, B, pick):
    """rpcc_ground_mask (with and without the tile table) + rpcc_fps_range at the cases of launch_variants.FPS_STAGE: pixels and centres
    equal the oracle's for every frame, and indices, centres and the final temp array equal the brute-force kernel's.  The brute-force
    stage entry loads 16 bytes at frame bases, so it refuses a pixel count that is no multiple of four (RPCC_ERR_ARG, as
    include/rpcc_hip.h states): at those shapes that refusal is pinned, and the two pruned runs are compared with each other."""
    torch, ops = env["torch"], env["ops"]
    assert lv.fps_pick_range(H, W, B, 0, None, False) == pick
    M = lv.default_m(H, W)
    g, geom, tm = _geom(env, H, W)
    xyz, offs, fid, scenes = _batch(env, H, W, B)
    exp = _oracle_scenes(H, W, lv.n_scenes(H, W, B), M)
    d_tm = _to(env, tm)
    ri = ops.project(xyz, offs, geom)
    gms, _ = ops.ground_ransac(ri, d_tm, seed=SEED, frame_ids=fid)
    res = {mode: _stage_fps(env, ri, d_tm, gms, M, mode) for mode in ("tiled", "tiled+table")}
    if (H * W) % 4 == 0:
        res["brute"] = _stage_fps(env, ri, d_tm, gms, M, "brute")
    else:
        with pytest.raises(env["lib"].RpccError, match=r"code -1"):
            _stage_fps(env, ri, d_tm, gms, M, "brute")
    torch.cuda.synchronize()
    assert _beq(_np(gms), np.stack([exp[k]["gm"] for k in scenes]))
    base = res.get("brute", res["tiled"])
    for mode in ("tiled", "tiled+table"):
        for a, b, what in zip(base, res[mode], ("indices", "centres", "temp")):
            assert np.array_equal(a, b), (mode, what, np.flatnonzero((a != b).reshape(B, -1).any(1))[:8])
    for i, k in enumerate(scenes):
        assert np.array_equal(res["tiled"][0][i], exp[k]["pix"]), (i, "FPS pixels")
        assert np.array_equal(res["tiled"][1][i], exp[k]["cen"].view(np.uint32)), (i, "centres")


# ------------------------------------------------------------------------------------------------
# FPS: lists
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,B,image,pick", lv.FPS_LISTS, ids=["%d-%d" % c[:2] for c in lv.FPS_LISTS])
def test_list_entry_fps_variants(env, N, B, image, pick):
    """rpcc_fps_xyz on B lists per call (launch_variants.FPS_LISTS): row-major non-empty pixels of synthetic images, which the probe marks
    coherent (the pruned kernel), and one shuffled list, which it hands to the one-pass kernel in the same call.  Indices and the final temp
    equal the brute-force entry's; the indices equal orc.fps on every distinct list."""
    torch, ops, orc = env["torch"], env["ops"], env["orc"]
    assert lv.fps_pick_list(N, B) == pick
    H, W = image
    n = lv.n_scenes(H, W, B)
    lists = [lv.list_points(H, W, k, N) for k in range(n)]
    scenes = [lv.scene_of(i, n) for i in range(B)]
    shuffled = lists[scenes[-1]][np.random.default_rng(N).permutation(N)]
    pts = np.stack([lists[k] for k in scenes[:-1]] + [shuffled])
    d_pts = _to(env, pts)
    marks = _np(ops.fps_xyz_probe(d_pts))
    assert (marks[:-1] == 0).all() and marks[-1] == -1, marks
    out = {}
    for brute in (False, True):
        temp = torch.full((B, N), 1e10, dtype=torch.float32, device=env["dev"])
        assert d_pts.data_ptr() % 16 == 0 and temp.data_ptr() % 16 == 0
        idx = ops.fps_xyz(d_pts, lv.LIST_M, temp=temp, bruteforce=brute)
        out[brute] = (_np(idx), _np(temp).view(np.uint32))
    assert np.array_equal(out[False][0], out[True][0]), np.flatnonzero((out[False][0] != out[True][0]).any(1))[:8]
    assert np.array_equal(out[False][1], out[True][1]), np.flatnonzero((out[False][1] != out[True][1]).any(1))[:8]
    exp = [orc.fps(lists[k], lv.LIST_M) for k in range(n)]
    exp_shuffled = orc.fps(shuffled, lv.LIST_M)
    assert len(set(exp_shuffled.tolist())) == lv.LIST_M
    for i, k in enumerate(scenes[:-1]):
        assert np.array_equal(out[False][0][i], exp[k]), i
    assert np.array_equal(out[False][0][-1], exp_shuffled)


# ------------------------------------------------------------------------------------------------
# FPS: the mixed call
# ------------------------------------------------------------------------------------------------
def _mixed_groups(env, table, offset_group=None):
    torch, ops = env["torch"], env["ops"]
    groups, meta = [], []
    for j, (H, W, B, _, _) in enumerate(table):
        g, geom, tm = _geom(env, H, W)
        xyz, offs, fid, scenes = _batch(env, H, W, B)
        buf = ops.BatchBuffers(B, geom, lv.MIXED_M, env["dev"], max_points=int(xyz.shape[0]))
        d_tm = _to(env, tm)
        if j == offset_group:
            buf.ri, buf.seg, d_tm = _offset_view(env, buf.ri, 16), _offset_view(env, buf.seg, 4), _offset_view(env, d_tm, 16)
        groups.append(dict(xyz=xyz, offsets=offs, tm=d_tm, ground=torch.zeros((B, 4), dtype=torch.float64, device=env["dev"]), buf=buf,
                           ground_seed=SEED, frame_ids=fid))
        meta.append((H, W, B, scenes))
    return groups, meta


_FIELDS = ("ri", "seg", "cen_pix", "centers", "model", "counts", "nnz")


def _same_outputs(a, b, tag):
    """Two runs of one batch: every output buffer, and the integers up to nnz."""
    assert _beq(_np(a["ground"]), _np(b["ground"])), (tag, "ground")
    for f in _FIELDS:
        assert _beq(_np(getattr(a["buf"], f)), _np(getattr(b["buf"], f))), (tag, f)
    nz, qa, qb = _np(a["buf"].nnz), _np(a["buf"].q16), _np(b["buf"].q16)
    assert all(np.array_equal(qa[i, :nz[i]], qb[i, :nz[i]]) for i in range(a["buf"].B)), (tag, "q16")


@pytest.mark.parametrize("table", [lv.FPS_MIXED, lv.FPS_MIXED_SMALL], ids=["130-frames", "6-frames"])
def test_mixed_call_fps_variants(env, table):
    """One rpcc_compress_batch_mixed (launch_variants.FPS_MIXED: 60 frames of 7 x 301 and 40 of 8 x 512 share
    fps_regtab_planar_multi_kernel<512>, one group with the EDGE flag and one without; 30 frames of 9 x 8209 would take planar2 in a
    launch of 130 frames, leave the common launch and run alone): every output of every group equals the same group through
    rpcc_compress_batch alone -- at most 128 frames, the 1024-thread kernels: two instantiations against each other -- and the oracle."""
    torch, ops = env["torch"], env["ops"]
    picks = lv.mixed_fps_picks([(H, W, B, lv.range_quads16(W)) for (H, W, B, _, _) in table])
    assert picks == [(c, k) for (_, _, _, c, k) in table]
    alone, meta = _mixed_groups(env, table)
    for a in alone:
        ops.compress_batch(**a)
    mixed, _ = _mixed_groups(env, table)
    ops.compress_batch_mixed(mixed)
    torch.cuda.synchronize()
    for j, (a, m, (H, W, B, scenes)) in enumerate(zip(alone, mixed, meta)):
        _same_outputs(a, m, ("group", j))
        exp = _oracle_scenes(H, W, lv.n_scenes(H, W, B), lv.MIXED_M)
        _check_all(m["buf"], m["ground"], exp, scenes, ("mixed group", j))


# ------------------------------------------------------------------------------------------------
# data arrays at their natural alignment
# ------------------------------------------------------------------------------------------------
def _offset_view(env, t, align):
    """A contiguous tensor of t's shape, dtype and content that starts one element into a larger (256-byte aligned) tensor: aligned for
    its element type and not for `align` bytes."""
    torch = env["torch"]
    big = torch.empty(t.numel() + 64, dtype=t.dtype, device=t.device)
    assert big.data_ptr() % 256 == 0
    v = big[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % t.element_size() == 0 and v.data_ptr() % align != 0
    return v


@pytest.mark.parametrize("H,W", lv.ALIGN_SHAPES)
@pytest.mark.parametrize("which", ["ri", "tm", "ri+tm", "seg"])
def test_fused_entry_with_arrays_at_natural_alignment(env, H, W, which):
    """rpcc_compress_batch with buf.ri, tm (range_quads16: the FPS, the mask) and buf.seg (hist_vec, quantise_vec: 4-byte label quads) one
    element into a larger tensor: the same outputs as with 256-byte aligned arrays, and the oracle's."""
    torch, ops = env["torch"], env["ops"]
    B, M = 2, lv.default_m(H, W)
    g, geom, tm = _geom(env, H, W)
    xyz, offs, fid, scenes = _batch(env, H, W, B)
    exp = _oracle_scenes(H, W, B, M)
    runs = []
    for offset in (False, True):
        buf = ops.BatchBuffers(B, geom, M, env["dev"], max_points=int(xyz.shape[0]))
        d_tm = _to(env, tm)
        for t in (buf.ri, buf.seg, d_tm):
            assert t.data_ptr() % 256 == 0
        if offset:
            if "ri" in which:
                buf.ri = _offset_view(env, buf.ri, 16)
            if "tm" in which:
                d_tm = _offset_view(env, d_tm, 16)
            if which == "seg":
                buf.seg = _offset_view(env, buf.seg, 4)
        run = dict(buf=buf, ground=torch.zeros((B, 4), dtype=torch.float64, device=env["dev"]))
        ops.compress_batch(xyz, offs, d_tm, run["ground"], buf, ground_seed=SEED, frame_ids=fid)
        torch.cuda.synchronize()
        _check_all(buf, run["ground"], exp, scenes, (H, W, which, "offset" if offset else "aligned"))
        runs.append(run)
    _same_outputs(runs[0], runs[1], (H, W, which))


def test_mixed_call_with_one_group_at_natural_alignment(env):
    """One mixed call in which the first group's ri, tm and seg are offset views and the second's are not (the multi kernels decide per
    group: m.edge, a.vec): the outputs of the call with every array aligned, and the oracle's."""
    torch, ops = env["torch"], env["ops"]
    table = [(8, 512, 3, True, None), (5, 300, 2, True, None), (8, 512, 2, True, None)]
    aligned, meta = _mixed_groups(env, table)
    ops.compress_batch_mixed(aligned)
    offset, _ = _mixed_groups(env, table, offset_group=0)
    assert offset[0]["buf"].ri.data_ptr() % 16 == 4 and offset[0]["tm"].data_ptr() % 16 == 4 and offset[0]["buf"].seg.data_ptr() % 4 == 1
    assert offset[2]["buf"].ri.data_ptr() % 16 == 0 and offset[2]["buf"].seg.data_ptr() % 4 == 0
    ops.compress_batch_mixed(offset)
    torch.cuda.synchronize()
    for j, (a, m, (H, W, B, scenes)) in enumerate(zip(aligned, offset, meta)):
        _same_outputs(a, m, ("group", j))
        _check_all(m["buf"], m["ground"], _oracle_scenes(H, W, lv.n_scenes(H, W, B), lv.MIXED_M), scenes, ("offset group", j))


@pytest.mark.parametrize("H,W", lv.ALIGN_SHAPES)
@pytest.mark.parametrize("which", ["ri", "tm", "temp"])
def test_mask_and_fps_stage_entries_at_natural_alignment(env, H, W, which):
    """rpcc_ground_mask (with and without the tile table) and rpcc_fps_range with ri, tm or temp one float into a larger tensor: temp,
    info, FPS pixels and centres equal the aligned run's, and the pixels and centres the oracle's."""
    torch, ops, L = env["torch"], env["ops"], env["lib"]
    B, M = 2, lv.default_m(H, W)
    g, geom, tm = _geom(env, H, W)
    xyz, offs, fid, scenes = _batch(env, H, W, B)
    exp = _oracle_scenes(H, W, B, M)
    ri0 = ops.project(xyz, offs, geom)
    gms, _ = ops.ground_ransac(ri0, _to(env, tm), seed=SEED, frame_ids=fid)
    res = {}
    for table in (False, True):
        for offset in (False, True):
            ri, d_tm = ri0.clone(), _to(env, tm)
            temp = torch.empty((B, H * W), dtype=torch.float32, device=env["dev"])
            if offset:
                ri = _offset_view(env, ri, 16) if which == "ri" else ri
                d_tm = _offset_view(env, d_tm, 16) if which == "tm" else d_tm
                temp = _offset_view(env, temp, 16) if which == "temp" else temp
            assert (ri.data_ptr() % 16 == 0) == (not (offset and which == "ri")) and (temp.data_ptr() % 16 == 0) == (not (offset and which == "temp"))
            info = torch.empty((B, L.INFO_INTS), dtype=torch.int32, device=env["dev"])
            tab = torch.empty(L.lib().rpcc_fps_table_bytes(B, H, W) // 4, dtype=torch.float32, device=env["dev"]) if table else None
            L.check(L.lib().rpcc_ground_mask(L.ptr(ri), L.ptr(d_tm), L.ptr(gms), 0.1, B, H, W, L.ptr(temp), L.ptr(info), L.ptr(tab), L.stream()))
            pix, cen = ops.fps_range(ri, d_tm, temp, info, M, fps_table=tab)
            torch.cuda.synchronize()
            res[(table, offset)] = (_np(pix), _np(cen), _np(temp), _np(info)[:, [0, 1, 2, 4]])     # (info[3] is the table flag)
    for key, r in res.items():
        for a, b, what in zip(res[(False, False)], r, ("pixels", "centres", "temp", "info")):
            assert _beq(a, b), (key, what)
        for i, k in enumerate(scenes):
            assert np.array_equal(r[0][i], exp[k]["pix"]) and _beq(r[1][i], exp[k]["cen"]), (key, i)


def _model_and_quantise(env, ri, d_tm, seg, gms, M, residual=None):
    """rpcc_point_model + rpcc_predict_quantize, or their _wide twins on uint16 labels -> (model, q16, nnz)."""
    torch, L = env["torch"], env["lib"]
    B, P = ri.shape[0], ri[0].numel()
    wide = seg.dtype == torch.uint16
    nbytes = L.lib().rpcc_wide_workspace_bytes(B, P, M, 0) if wide else L.lib().rpcc_workspace_bytes(B, P, M, 0)
    ws = torch.empty((nbytes + 255) // 256 * 256, dtype=torch.uint8, device=env["dev"])
    model = torch.empty((B, M + 2, 4), dtype=torch.float32, device=env["dev"])
    counts = torch.empty((B, M + 2), dtype=torch.int32, device=env["dev"])
    q = torch.zeros((B, P), dtype=torch.int16, device=env["dev"])
    nnz = torch.empty((B,), dtype=torch.int32, device=env["dev"])
    sfx = "_wide" if wide else ""
    L.check(getattr(L.lib(), "rpcc_point_model" + sfx)(L.ptr(ri), L.ptr(seg), L.ptr(gms), B, P, M, L.ptr(model), L.ptr(counts), L.ptr(ws), L.stream()))
    L.check(getattr(L.lib(), "rpcc_predict_quantize" + sfx)(L.ptr(ri), L.ptr(d_tm), L.ptr(seg), L.ptr(model), None, L.ptr(residual), 0.04, B, P, M,
                                                            L.ptr(q), None, L.ptr(nnz), None, L.ptr(ws), L.stream()))
    torch.cuda.synchronize()
    return _np(model), _np(q), _np(nnz)


@pytest.mark.parametrize("H,W", lv.ALIGN_SHAPES)
@pytest.mark.parametrize("which", ["seg", "seg16", "residual", "residual+seg"])
def test_model_and_quantiser_stage_entries_at_natural_alignment(env, H, W, which):
    """rpcc_point_model and rpcc_predict_quantize (and their _wide twins on uint16 labels) with the labels one element into a larger
    tensor (1 byte, 2 bytes: not aligned for a quad of labels), and rpcc_predict_quantize with the caller's residual one float into one:
    model rows and quantised integers equal the aligned run's and the oracle's."""
    torch, ops = env["torch"], env["ops"]
    B, M = 2, lv.default_m(H, W)
    g, geom, tm = _geom(env, H, W)
    exp = _oracle_scenes(H, W, B, M)
    ri = _to(env, np.stack([o["ri"].reshape(H, W) for o in exp]))
    d_tm = _to(env, tm)
    gms = _to(env, np.stack([o["gm"] for o in exp]))
    seg = _to(env, np.stack([o["seg"].reshape(H, W) for o in exp]).astype(np.uint16 if which == "seg16" else np.uint8))
    residual = None
    if "residual" in which:      # the quantiser's own seam: ri - pred handed in by the caller
        model = _to(env, np.stack([np.concatenate([o["model"], np.zeros((M + 2 - o["model"].shape[0], 4), np.float32)]) for o in exp]))
        residual = (ri - ops.intra_predict(seg, model, d_tm)).reshape(B, -1).contiguous()
    runs = []
    for offset in (False, True):
        s, r = seg, residual
        if offset and "seg" in which:
            s = _offset_view(env, seg, 8 if which == "seg16" else 4)
        if offset and "residual" in which:
            r = _offset_view(env, residual, 16)
        runs.append(_model_and_quantise(env, ri, d_tm, s, gms, M, r))
    for (model, q, nnz) in runs:
        for i, o in enumerate(exp):
            nrow = o["model"].shape[0]
            assert _beq(model[i, :nrow], o["model"]), (which, i, "model rows")
            assert int(nnz[i]) == o["q"].shape[0] and np.array_equal(q[i, :nnz[i]], o["q"]), (which, i, "quantised integers")
    assert _beq(runs[0][0], runs[1][0]) and np.array_equal(runs[0][2], runs[1][2])


@pytest.mark.parametrize("which", ["points", "temp"])
def test_list_entry_at_natural_alignment(env, which):
    """rpcc_fps_xyz with N a multiple of four and the point list or temp one float into a larger tensor (the `vec` test of fps_xyz_impl):
    indices and the final temp equal the aligned run's, and the indices orc.fps's."""
    torch, ops, orc = env["torch"], env["ops"], env["orc"]
    N, B = lv.ALIGN_LIST_N, 3
    assert N % 4 == 0
    lists = [lv.list_points(8, 32768, k, N) for k in range(B)]
    lists[-1] = lists[-1][np.random.default_rng(5).permutation(N)]          # one list for the one-pass kernel
    pts = _to(env, np.stack(lists))
    marks = _np(ops.fps_xyz_probe(pts))
    assert (marks[:-1] == 0).all() and marks[-1] == -1, marks          # both kernels run in each call
    runs = []
    for offset in (False, True):
        p = _offset_view(env, pts, 16) if offset and which == "points" else pts
        temp = torch.full((B, N), 1e10, dtype=torch.float32, device=env["dev"])
        temp = _offset_view(env, temp, 16) if offset and which == "temp" else temp
        assert (p.data_ptr() % 16 == 0 and temp.data_ptr() % 16 == 0) == (not offset)
        assert np.array_equal(_np(ops.fps_xyz_probe(p)), marks)
        idx = ops.fps_xyz(p, lv.LIST_M, temp=temp)
        runs.append((_np(idx), _np(temp)))
    assert _beq(runs[0][0], runs[1][0]) and _beq(runs[0][1], runs[1][1])
    for i in range(B):
        assert np.array_equal(runs[1][0][i], orc.fps(lists[i], lv.LIST_M)), i


# ------------------------------------------------------------------------------------------------
# key-point features
# ------------------------------------------------------------------------------------------------
def _features(env, c, dtype, nlab):
    ops, orc = env["ops"], env["orc"]
    W, params = c[0], c[1:6]
    seg, ri = lv.feature_image(W, params, nlab=nlab)
    f_o, k_o = orc.extract_features_with_segment(ri, seg, *params)
    assert k_o.max() >= 1
    feat, kp = ops.extract_features(_to(env, ri[None]), _to(env, seg.astype(dtype)[None]), *params)
    assert np.array_equal(_np(kp[0]), k_o.astype(np.uint8)), (c, "key-point map", np.argwhere(_np(kp[0]) != k_o)[:8])
    assert _beq(_np(feat[0]), f_o), (c, "curvature image")


@pytest.mark.parametrize("case", lv.FEATURE_CASES, ids=["%d-%d-%d-%d-%d-%d" % c[:6] for c in lv.FEATURE_CASES])
def test_feature_classes_and_boundaries(env, case):
    """rpcc_extract_features (curvature image, uint8 labels) in every chunk-length class at both widths per wavefront, with both sides of
    every class boundary (launch_variants.FEATURE_CASES): key-point map and curvature image equal the oracle's."""
    assert lv.feature_pick(case[0], case[1], case[2], case[5]) == case[6] + (False,)
    _features(env, case, np.uint8, 20)


@pytest.mark.parametrize("case", lv.FEATURE_CASES_WIDE, ids=["%d-%d-%d-%d-%d-%d" % c[:6] for c in lv.FEATURE_CASES_WIDE])
def test_feature_classes_on_uint16_labels(env, case):
    """The same classes through rpcc_extract_features_wide, on labels that need uint16."""
    _features(env, case, np.uint16, 600)


def test_features_refuse_a_row_wider_than_a_workgroup_covers(env):
    """W = 4097: more than 64 * FEAT_GPW columns per wavefront -- RPCC_ERR_ARG."""
    ops = env["ops"]
    W = lv.FEATURE_REFUSED_W
    seg, ri = lv.feature_image(W, (3, 8, 4, 8, 6))
    with pytest.raises(env["lib"].RpccError, match=r"code -1"):
        ops.extract_features(_to(env, ri[None]), _to(env, seg.astype(np.uint8)[None]))


@pytest.mark.parametrize("lidar,kp,pick", lv.FEATURE_FUSED, ids=["%s-%d" % (c[0], c[1]["segments"]) for c in lv.FEATURE_FUSED])
def test_fused_nonuniform_entry_feature_forms(env, lidar, kp, pick):
    """The fused non-uniform entry (no curvature image): the compact row-mode form at W = 1800 (G = 8) and W = 2250 (G = 16), and the full
    form of a register class with the curvature pointer NULL.  Key-point map, salience levels and quantised integers equal the oracle's."""
    torch, ops, orc, dev = env["torch"], env["ops"], env["orc"], env["dev"]
    from rpcc_amd import synth
    gd = orc.GEOMS[lidar]
    g = orc.LidarGeom(**gd)
    assert lv.feature_pick(g.W, kp["feature_region"], kp["segments"], kp["flat_num"], feat=False) == pick
    tm = orc.transform_map(g)
    geom = ops.make_geom(g.H, g.W, g.horizontal_FOV, g.vertical_max, g.vertical_min)
    ids = [7100, 7101]
    frames = [synth.make_frame(i, g.H, g.W, vmax_deg=gd["vmax_deg"], vmin_deg=gd["vmin_deg"]).numpy() for i in ids]
    offs = np.zeros(len(frames) + 1, np.int64)
    offs[1:] = np.cumsum([f.shape[0] for f in frames])
    cfg = dict(orc.DEFAULT_CFG, **kp)
    buf = ops.BatchBuffers(len(ids), geom, 100, dev, general=True)
    gms = torch.zeros((len(ids), 4), dtype=torch.float64, device=dev)
    ops.compress_batch(_to(env, np.concatenate(frames)), _to(env, offs), _to(env, tm), gms, buf, ground_seed=SEED, frame_ids=ids,
                       nonuniform=ops.nonuniform_cfg(0.04, cfg))
    torch.cuda.synchronize()
    q16, nnz = _np(buf.q16), _np(buf.nnz)
    for i, f in enumerate(frames):
        gm = orc.ground_model(orc.project(f, g), tm, seed=SEED + ids[i])
        assert _beq(_np(gms[i]), np.asarray(gm, np.float64))
        o = orc.compress_frame(f, g, tm, gm, cfg, uniform=False)
        assert len(set(o["fps_pix"].tolist())) == 100 and o["key_point_map"].max() >= 1
        assert np.array_equal(_np(buf.seg[i]), o["seg_idx"].astype(np.uint8)), (i, "labels")
        assert np.array_equal(_np(buf.key_point_map[i]), o["key_point_map"].astype(np.uint8)), (i, "key-point map")
        assert np.array_equal(_np(buf.salience[i, :o["salience"].shape[0]]), o["salience"].astype(np.uint8)), (i, "salience levels")
        n = int(nnz[i])
        assert n == o["q"].shape[0] and np.array_equal(q16[i, :n], o["q"].astype(np.int16)), (i, "quantised integers")


# ------------------------------------------------------------------------------------------------
# assignment
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,nbytes,rounds", lv.ASSIGN_CASES)
def test_assignment_at_the_label_type_and_round_switches(env, M, nbytes, rounds):
    """rpcc_assign at M = 254 (the last byte-label count) and rpcc_assign_wide at 255, 510 (8 screening rounds) and 511 (16), on one
    16 x 1800 frame with M distinct centres: labels equal the oracle's."""
    torch, ops, orc = env["torch"], env["ops"], env["orc"]
    assert (lv.label_bytes(M), lv.assign_rounds(lv.label_bytes(M), M)) == (nbytes, rounds)
    H, W = lv.ASSIGN_SHAPE
    g, geom, tm = _geom(env, H, W)
    ri = orc.project(lv.scene_frame(H, W, 0), g)
    gm = np.asarray(orc.ground_model(ri, tm, seed=SEED), np.float64)
    s = orc.segment(ri, tm, gm, dict(orc.DEFAULT_CFG, cluster_num=M))
    assert len(set(s["fps_pix"].tolist())) == M
    seg = ops.assign(_to(env, ri[None]), _to(env, tm), _to(env, gm[None]), _to(env, s["centers"].astype(np.float32)[None]))
    assert seg.element_size() == nbytes
    got = _np(seg[0]).astype(np.int64)
    bad = np.flatnonzero(got.reshape(-1) != s["seg_idx"].reshape(-1))
    assert bad.size == 0, (M, bad[:8], got.reshape(-1)[bad[:8]], s["seg_idx"].reshape(-1)[bad[:8]])
    assert nbytes == 1 or got.max() > 255         # the frame does use the labels past a byte
