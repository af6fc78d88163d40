"""The projection through a per-beam elevation table on the GPU (rpcc_project_beams, rpcc_compress_batch_beams, PCTransformer(cfg, csv)),
every result compared by bits with the specification (tests/beam_table_ref.py) or with the existing stage entries run on the same image."""
import math
import os

import numpy as np
import pytest

import beam_table_ref as R
import grid_caps as GC
from beam_table_cases import HFOV, constructed as _constructed, past_the_grid as _past_the_grid, tables as _tables
from buffer_arena import Arena, filled

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CFG = os.path.join(ROOT, "r-pcc_amd", "lidar_cfg")
YAML, CSV = os.path.join(CFG, "Velodyne_HDL_64E.yaml"), os.path.join(CFG, "Velodyne_HDL_64E_beams.csv")
POISON = 0xCD


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    import __graft_entry__ as ge
    ge.build()
    import rpcc_amd  # noqa: F401
    from rpcc_amd import _lib, ops
    dev = torch.device("cuda:0")
    xyz = np.ascontiguousarray(np.load(os.path.join(HERE, "golden", "example_64E.npz"))["xyz"], dtype=np.float32)
    va = R.read_csv(CSV)
    e = dict(torch=torch, ops=ops, lib=_lib, dev=dev, xyz=xyz, va=va, golden=np.load(os.path.join(HERE, "golden", "beam_table_example_64E.npz")),
             geom=ops.make_geom(64, 2000, HFOV, 0.0, 0.0), beams=ops.beam_index(va, dev), cache={})
    return e


def _to(env, a):
    return env["torch"].from_numpy(np.ascontiguousarray(a)).to(env["dev"])


def _beq(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _offsets(frames):
    o = np.zeros(len(frames) + 1, np.int64)
    o[1:] = np.cumsum([f.shape[0] for f in frames])
    return o


def _project(env, frames, va, H, W, rows16=False, **kw):
    ops = env["ops"]
    pts = np.concatenate(frames) if len(frames) else np.zeros((0, 3), np.float32)
    if rows16:
        pts = np.concatenate([pts, np.full((pts.shape[0], 1), 0.5, np.float32)], 1)
    geom = ops.make_geom(H, W, HFOV, 0.0, 0.0)
    return ops.project(_to(env, pts), _to(env, _offsets(frames)), geom, beams=ops.beam_index(va, env["dev"]), **kw).cpu().numpy()


def _frames4(env, W=2000):
    """Four sweeps from the example: as stored, every second point, rotated about z, its tail; and their reference image at width W."""
    if ("frames4", W) not in env["cache"]:
        x = env["xyz"]
        c, s = np.float32(math.cos(0.1)), np.float32(math.sin(0.1))
        rot = np.stack([c * x[:, 0] - s * x[:, 1], s * x[:, 0] + c * x[:, 1], x[:, 2]], 1).astype(np.float32)
        fr = [x, np.ascontiguousarray(x[::2]), rot, np.ascontiguousarray(x[30000:])]
        env["cache"]["frames4", W] = (fr, R.project_batch(np.concatenate(fr), _offsets(fr), env["va"], HFOV, 64, W))
    return env["cache"]["frames4", W]


# ------------------------------------------------------------------------------------------------
# the example sweep against the genuine reference's table branch
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows16", (False, True))
def test_example_sweep_equals_the_golden(env, rows16):
    ri = _project(env, [env["xyz"]], env["va"], 64, 2000, rows16=rows16)
    assert _beq(ri[0], env["golden"]["ri"])


def test_batch_with_an_empty_middle_frame(env):
    x = env["xyz"]
    fr = [np.ascontiguousarray(x[:40000]), np.zeros((0, 3), np.float32), np.ascontiguousarray(x[-30000:])]
    ri = _project(env, fr, env["va"], 64, 2000)
    want = R.project_batch(np.concatenate(fr), _offsets(fr), env["va"], HFOV, 64, 2000)
    assert _beq(ri, want) and not ri[1].any() and ri[0].any() and ri[2].any()
    assert not _project(env, [np.zeros((0, 3), np.float32)], env["va"], 64, 2000).any()       # a call without points: an empty image


def test_transformer_and_integration_binding(env):
    from rpcc_amd.transformer import PCTransformer
    T = PCTransformer(YAML, CSV)
    assert _beq(T.point_cloud_to_range_image(env["xyz"]), env["golden"]["ri"])
    assert _beq(T.point_cloud_to_range_image(np.concatenate([env["xyz"], np.ones((env["xyz"].shape[0], 1), np.float32)], 1)), env["golden"]["ri"])
    import importlib.util
    spec = importlib.util.spec_from_file_location("rpcc_hip_binding", os.path.join(ROOT, "integration", "rpcc_hip_binding.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert _beq(mod.point_cloud_to_range_image_table(env["xyz"], 64, 2000, T.horizontal_FOV, T.vertical_angle), env["golden"]["ri"])


# ------------------------------------------------------------------------------------------------
# constructed sets
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", (8, 64))
@pytest.mark.parametrize("H", (1, 2, 5))
def test_constructed_sets(env, H, W):
    ops = env["ops"]
    for name, (va, tie) in _tables(H).items():
        xyz = _constructed(va, W, tie)
        last0 = np.concatenate([xyz, np.array([[7.0, 0.0, 0.0], [0.0, 0.0, 0.0]], np.float32)])    # ... and with a (0,0,0) point last
        for tag, pts in (("base", xyz), ("zero last", last0)):
            want = R.project(pts, va, HFOV, H, W)
            got = _project(env, [pts], va, H, W)[0]
            assert _beq(got, want), (name, tag, np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:5])
        keep, row, col, _ = R.pixels(last0, va, HFOV, W)
        assert R.project(last0, va, HFOV, H, W)[row[-1], col[-1]] == 0 and col[-1] == 0
        if tie is not None:      # the tie is exact in fp64 and goes to the lower ROW
            k, r, _, _ = R.pixels(tie[None], va, HFOV, W)
            d = np.abs(va - float(R.atan2f(tie[2:3], np.sqrt(tie[0:1] ** 2 + tie[1:2] ** 2))[0]))
            assert (d == d.min()).sum() == 2 and r[0] == np.flatnonzero(d == d.min())[0]
        geom = ops.make_geom(H, W, HFOV, 0.0, 0.0)
        sure, bad, slow = ops.project_beams_check(_to(env, last0), geom, ops.beam_index(va, env["dev"]))
        assert bad == 0 and sure + slow == last0.shape[0], (name, sure, bad, slow)


# ------------------------------------------------------------------------------------------------
# the fast path never disagrees with the exact sequence
# ------------------------------------------------------------------------------------------------
def _seeded_points(env, n, seed, lo, hi):
    torch = env["torch"]
    g = torch.Generator(device=env["dev"])
    g.manual_seed(seed)
    u = torch.rand((n, 3), generator=g, device=env["dev"], dtype=torch.float64)
    az, el, r = u[:, 0] * (2 * math.pi), lo - 0.05 + u[:, 1] * (hi - lo + 0.1), 0.5 + u[:, 2] * 100
    return torch.stack([r * torch.cos(el) * torch.cos(az), r * torch.cos(el) * torch.sin(az), r * torch.sin(el)], 1).to(torch.float32).contiguous()


def test_fast_path_never_disagrees(env):
    ops = env["ops"]
    n = env["xyz"].shape[0]
    sure, bad, slow = ops.project_beams_check(_to(env, env["xyz"]), env["geom"], env["beams"])
    print("example sweep: %d certain, %d disagree, %d exact (%.2f %%)" % (sure, bad, slow, 100.0 * slow / n))
    assert bad == 0 and sure + slow == n and sure > 0.9 * n
    rng = np.random.default_rng(11)
    geoms = {"64x2000 shipped": (env["va"], 2000), "16x1800 uneven": (np.sort(rng.uniform(-0.3, 0.3, 16)), 1800),
             "128x512 shuffled": (rng.permutation(np.cumsum(rng.uniform(0.001, 0.008, 128)) - 0.4), 512), "5x64": (_tables(5)["shuffled"][0], 64)}
    for k, (name, (va, W)) in enumerate(geoms.items()):
        pts = _seeded_points(env, 1_000_000, 100 + k, float(va.min()), float(va.max()))
        sure, bad, slow = ops.project_beams_check(pts, ops.make_geom(len(va), W, HFOV, 0.0, 0.0), ops.beam_index(va, env["dev"]))
        print("%s: %d certain, %d disagree, %d exact" % (name, sure, bad, slow))
        assert bad == 0 and sure + slow == 1_000_000 and sure > 500_000, name


# ------------------------------------------------------------------------------------------------
# caller's buffers
# ------------------------------------------------------------------------------------------------
def test_scratch_of_exact_size_with_any_contents(env):
    ops, torch = env["ops"], env["torch"]
    x = env["xyz"]
    sets = [[np.ascontiguousarray(x[:50000]), np.ascontiguousarray(x[50000:90000])], [np.ascontiguousarray(x[60000:])]]
    want = [R.project_batch(np.concatenate(f), _offsets(f), env["va"], HFOV, 64, 2000) for f in sets]
    need = [int(env["lib"].lib().rpcc_project_beams_scratch_bytes(sum(p.shape[0] for p in f), len(f), 64 * 2000)) for f in sets]
    arena = Arena(max(need), env["dev"])

    def run(k):
        f = sets[k]
        out = filled((len(f), 64, 2000), torch.float32, env["dev"], POISON)
        ri = ops.project(_to(env, np.concatenate(f)), _to(env, _offsets(f)), env["geom"], ri=out, scratch=arena.first(need[k]), beams=env["beams"])
        assert _beq(ri.cpu().numpy(), want[k]), k
        assert arena.check_guards() is None

    for pattern in ("ones", "zero", "nan", "alt(0,1)"):
        arena.fill(pattern)
        run(0)
        run(1)        # ... on what the call before left there, under another B and point count
        run(0)


# ------------------------------------------------------------------------------------------------
# past the grid caps: two trips of every loop, the LDS queue carried from one to the next (tests/grid_caps.py, BT.past_the_grid;
# tests/test_beam_table_ref.py asserts on the CPU what the batch reaches)
# ------------------------------------------------------------------------------------------------
def _past(env):
    """The batch on the device (packed points and stored rows), and the reference image of every frame: one R.project per distinct frame."""
    if "past" not in env["cache"]:
        ops = env["ops"]
        c = _past_the_grid()
        per = np.stack([R.project(f, c["va"], HFOV, c["H"], c["W"]) for f in c["distinct"]])
        pts = np.concatenate(c["frames"])
        rows = np.concatenate([pts, np.full((pts.shape[0], 1), 0.5, np.float32)], 1)
        env["cache"]["past"] = dict(c, want=per[c["which"]], pts=_to(env, pts), rows=_to(env, rows), offs=_to(env, _offsets(c["frames"])),
                                    geom=ops.make_geom(c["H"], c["W"], HFOV, 0.0, 0.0), beams=ops.beam_index(c["va"], env["dev"]), total=pts.shape[0])
    return env["cache"]["past"]


def _assert_frames(got, p, tag):
    bad = np.flatnonzero((got.view(np.uint32) != p["want"].view(np.uint32)).reshape(got.shape[0], -1).any(1))
    assert got.shape == p["want"].shape and bad.size == 0, (tag, "frames", bad[:8].tolist(), "of kinds", p["which"][bad[:8]].tolist())


@pytest.mark.parametrize("rows16", (False, True))
def test_past_the_grid_equals_the_reference(env, rows16):
    ops = env["ops"]
    p = _past(env)
    assert p["total"] > GC.BEAMS_PIX_CAP * GC.BEAMS_CHUNK and p["total"] > GC.BEAMS_WRITE_CAP * GC.BEAMS_WRITE_THREADS
    assert p["want"].size > GC.BEAMS_FILL_CAP * GC.BEAMS_FILL_THREADS
    for tag in ("first", "again"):
        _assert_frames(ops.project(p["rows" if rows16 else "pts"], p["offs"], p["geom"], beams=p["beams"]).cpu().numpy(), p, (rows16, tag))
    zl, r0 = np.flatnonzero(p["which"] == 0), int(np.argmin(np.abs(p["va"])))
    assert not p["want"][zl, r0, 0].any() and p["want"][zl].any(axis=(1, 2)).all()     # (the zero that ends those frames leaves its pixel empty)
    if not rows16:
        sure, bad, slow = ops.project_beams_check(p["pts"], p["geom"], p["beams"])
        by_rule = int(sum((~p["aimed_fast"][k]).sum() for k in p["which"]))
        print("past the grid: %d points, %d certain, %d disagree, %d exact (%d aimed at the exact sequence)" % (p["total"], sure, bad, slow, by_rule))
        assert bad == 0 and sure + slow == p["total"] and slow >= by_rule


@pytest.mark.parametrize("pattern", ("ones", "alt(0,1)"))
def test_past_the_grid_scratch_of_exact_size(env, pattern):
    """... into a scratch of exactly the size asked for, filled with 0xFF (every remembered pixel reads as `skipped`, every maximum as -1) or
    with small positive words (every remembered pixel a pixel of the image): neither the fill kernel's second trip nor a point the queue
    lost may leave such a word in place."""
    ops, torch = env["ops"], env["torch"]
    p = _past(env)
    B, H, W = p["want"].shape
    need = int(env["lib"].lib().rpcc_project_beams_scratch_bytes(p["total"], B, H * W))
    arena = Arena(need, env["dev"])
    for rows16 in (False, True):
        arena.fill(pattern)
        out = filled((B, H, W), torch.float32, env["dev"], POISON)
        ri = ops.project(p["rows" if rows16 else "pts"], p["offs"], p["geom"], ri=out, scratch=arena.view, beams=p["beams"])
        _assert_frames(ri.cpu().numpy(), p, (pattern, rows16))
        assert arena.check_guards() is None


# ------------------------------------------------------------------------------------------------
# the fused call: the projection replaced, everything behind it as the stage entries give it
# ------------------------------------------------------------------------------------------------
ACC, THR, SEED = 0.04, 0.1, 3


@pytest.mark.parametrize("variant", ("uniform_point", "nonuniform_plane", "nonuniform_point", "uniform_plane"))
@pytest.mark.parametrize("M", (100, 300, 254))
def test_fused_batch(env, M, variant):
    """100 and 300 clusters (byte and uint16 labels) on the shipped 64 x 2000 image; 254 clusters on 64 x 3080 -- the table indexes rows, the
    width is free --: 193 scatter tiles, the last of 512 pixels, x 128 words, one tile past count_scan_kernel's LDS budget."""
    ops, torch, dev = env["ops"], env["torch"], env["dev"]
    B, H, W = 4, 64, 3080 if M == 254 else 2000
    frames, want_ri = _frames4(env, W)
    geom = ops.make_geom(H, W, HFOV, 0.0, 0.0)
    tm = _to(env, ops.transform_map(H, W, HFOV, 0.0, 0.0, vertical_angle=env["va"]))
    xyz, offs = _to(env, np.concatenate(frames)), _to(env, _offsets(frames))
    framework, method = variant.split("_")
    uniform = framework == "uniform"
    nu = None if uniform else ops.nonuniform_cfg(ACC)
    fid = [7, 8, 11, 2]
    buf = ops.BatchBuffers(B, geom, M, dev, max_points=xyz.shape[0], general=variant != "uniform_point")
    ground = filled((B, 4), torch.float64, dev, POISON)
    ops.compress_batch(xyz, offs, tm, ground, buf, THR, ACC, ground_seed=SEED, frame_ids=fid, model_method=method, plane_seed=SEED, nonuniform=nu,
                       beams=env["beams"])
    torch.cuda.synchronize()
    assert _beq(buf.ri.cpu().numpy(), want_ri)
    # the existing stage entries on that image and the table-built ray table
    ri = _to(env, want_ri)
    g2, _ = ops.ground_ransac(ri, tm, seed=SEED, frame_ids=fid)
    assert _beq(ground.cpu().numpy(), g2.cpu().numpy())
    temp, info, tab = ops.ground_mask(ri, tm, g2, THR, fps_table=True)
    cen_pix, centers = ops.fps_range(ri, tm, temp, info, M, fps_table=tab)
    assert np.array_equal(buf.cen_pix.cpu().numpy(), cen_pix.cpu().numpy()) and _beq(buf.centers.cpu().numpy(), centers.cpu().numpy())
    seg = ops.assign(ri, tm, g2, centers)
    assert seg.dtype == buf.seg.dtype and np.array_equal(buf.seg.cpu().numpy(), seg.cpu().numpy())
    if method == "point":
        model, counts = ops.point_model(ri, seg, g2, M)
    else:
        model, counts = ops.plane_model(ri, tm, seg, M, seed=SEED, ground=g2, want_counts=True, frame_ids=fid)
    assert _beq(buf.model.cpu().numpy(), model.cpu().numpy()) and np.array_equal(buf.counts.cpu().numpy(), counts.cpu().numpy())
    label_acc = None
    if not uniform:
        _, kp = ops.extract_features(ri, seg)
        lk = [nu.level_kp_num[i] for i in range(nu.levels)]
        la = np.array([nu.level_acc[i] for i in range(nu.levels)], dtype=np.float32)
        sal, label_acc = ops.salience(seg, kp, lk, la, nu.ground_level, M)
        assert np.array_equal(buf.key_point_map.cpu().numpy(), kp.cpu().numpy()) and np.array_equal(buf.salience.cpu().numpy(), sal.cpu().numpy())
    q, nnz, _ = ops.predict_quantize(ri, tm, seg, model, ACC, M, int16=True, label_acc=label_acc)
    nz, q_f, q_s = nnz.cpu().numpy(), buf.q16.cpu().numpy(), q.cpu().numpy()
    assert np.array_equal(buf.nnz.cpu().numpy(), nz) and nz.min() > 10000
    for b in range(B):
        assert np.array_equal(q_f[b, :nz[b]], q_s[b, :nz[b]]), b


# ------------------------------------------------------------------------------------------------
# front-ends: .rpcc containers and back
# ------------------------------------------------------------------------------------------------
def test_containers_round_trip_with_the_table(env, tmp_path):
    """BatchCompressor -> .rpcc -> BatchDecompressor and tools/decompress.py's decode_frame, all with the CSV: the same bytes, within the
    quantisation step of the specification's image; the same blob decoded WITHOUT the CSV gives another cloud (the table reaches the decoder
    through the transformer's ray table and through nothing else)."""
    from rpcc_amd.transformer import PCTransformer
    from rpcc_amd.pipeline import BatchCompressor, BatchDecompressor
    from rpcc_amd.compress_utils import BasicCompressor, unpack_bitstream
    from rpcc_amd.tools.decompress import decode_frame
    T, E = PCTransformer(YAML, CSV), PCTransformer(YAML)
    frames, want_ri = _frames4(env)
    frames, want_ri = frames[:2], want_ri[:2]
    accuracy = 0.04
    bc = BatchCompressor(T, cluster_num=100, accuracy=accuracy / 2, basic_compressor="bzip2", seed=1)
    blobs = bc.compress(frames, frame_ids=[4, 5])
    assert _beq(bc._buf.ri.cpu().numpy(), want_ri)
    out = BatchDecompressor(T, 100, accuracy).decompress(blobs)
    basic = BasicCompressor(method_name="bzip2")
    for b, blob in enumerate(blobs):
        rec, pc, seg = decode_frame(unpack_bitstream(blob, True), basic, T, 100, accuracy, None, True)
        assert _beq(out[b][0], rec) and _beq(out[b][1], pc) and np.array_equal(out[b][2], seg), b
        assert float(np.abs(rec - want_ri[b]).max()) <= accuracy + 1e-5
        assert _beq(pc, T.range_image_to_point_cloud(rec))
        _, pc_even, _ = decode_frame(unpack_bitstream(blob, True), basic, E, 100, accuracy, None, True)
        assert not _beq(pc, pc_even)
    # the DBSCAN front-end takes its projection from the same transformer
    db = BatchCompressor(T, segment_method="DBSCAN", accuracy=accuracy / 2, seed=1)
    xyz, offs, _, _ = db._upload(frames)
    db.compress_device(xyz, offs)
    env["torch"].cuda.synchronize()
    assert _beq(db._buf.ri.cpu().numpy(), want_ri)


def test_streaming_loader_takes_the_table_from_its_transformer(env):
    """loader.StreamingCompressor, both ingest modes: the .rpcc bytes of BatchCompressor.compress with the same transformer -- and not those of
    the even transformer."""
    from rpcc_amd.transformer import PCTransformer
    from rpcc_amd.pipeline import BatchCompressor
    from rpcc_amd.loader import StreamingCompressor
    T = PCTransformer(YAML, CSV)
    frames = _frames4(env)[0][:3]
    ids = [21, 22, 25]
    bc = BatchCompressor(T, accuracy=0.02, seed=9)
    want = bc.compress(frames, frame_ids=ids)
    assert BatchCompressor(PCTransformer(YAML), accuracy=0.02, seed=9).compress(frames[:1], frame_ids=ids[:1])[0] != want[0]
    rows = [np.concatenate([f, np.full((f.shape[0], 1), 0.25, np.float32)], 1) for f in frames]
    for src, kw in ((frames, {}), (rows, dict(ingest="rows"))):
        got = {}
        n = StreamingCompressor(bc, batch=2, depth=2, workers=2, **kw).run(((src[s:s + 2], ids[s:s + 2]) for s in (0, 2)),
                                                                          sink=lambda k, r: got.__setitem__(k, r))
        assert n == 3 and [b for k in sorted(got) for b in got[k]] == want, kw
