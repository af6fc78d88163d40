"""DBSCAN through the batch front-end on the MI355X: rpcc_compress_batch_labels against the stage entries it replaces (and the oracle), its
refusals, pipeline.BatchCompressor(segment_method="DBSCAN") against the per-frame stage sequence of tools/compress.py byte for byte, the
streaming loader and the datalist tools, and pipeline.BatchDecompressor on DBSCAN streams against decode_frame."""
import os

import numpy as np
import pytest

import labels_cases as LC

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 7
ACC = 0.04           # quantisation step (2 * accuracy)
COMBOS = (("uniform", "point"), ("uniform", "plane"), ("nonuniform", "point"), ("nonuniform", "plane"))
OUT_KEYS = ("seg", "counts", "model", "q", "nnz", "salience", "key_point_map")


@pytest.fixture(scope="module")
def env():
    import torch
    import __graft_entry__ as ge
    ge.build()
    from rpcc_amd import _lib, compress_utils, dbscan, ops, pipeline, synth
    from rpcc_amd.dataset import build_dataset
    from rpcc_amd.utils import load_compressor_cfg
    from rpcc_amd.tools.compress import PKG
    from oracle import oracle as orc
    assert torch.cuda.is_available()
    cfg = load_compressor_cfg(os.path.join(PKG, "cfgs/compressor.yaml"))
    return dict(torch=torch, lib=_lib, cu=compress_utils, db=dbscan, ops=ops, pl=pipeline, synth=synth, orc=orc, build_dataset=build_dataset,
                cfg=cfg, dev=torch.device("cuda:0"))


def dev(env, a):
    return env["torch"].from_numpy(np.ascontiguousarray(a)).to(env["dev"])


def bits(a):
    """Arrays compared bit for bit (NaN rows of empty labels, non-finite ranges)."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def labels_call(env, case, framework, model, ws=None, poison=None):
    """ops.compress_batch_labels on a case of labels_cases.batch -> per-frame dicts of numpy arrays and the status."""
    ops, torch = env["ops"], env["torch"]
    B, H, W = case["labels"].shape
    geom = ops.make_geom(H, W, 6.2831855, 0.03, -0.43)
    buf = ops.BatchBuffers(B, geom, case["cap"], env["dev"], general=(framework, model) != ("uniform", "point"), labels=True)
    if ws is not None:
        assert ws.numel() >= buf.ws.numel()
        buf.ws = ws
    if poison is not None:   # outputs hold garbage before the call: what comes back was written by it
        for t in (buf.seg, buf.model, buf.counts, buf.q16, buf.nnz, buf.status, buf.salience, buf.key_point_map):
            if t is not None:
                t.view(torch.uint8).fill_(poison)
    nu = ops.nonuniform_cfg(ACC, env["cfg"]) if framework == "nonuniform" else None
    st = ops.compress_batch_labels(dev(env, case["ri"]), dev(env, case["tm"]), dev(env, case["ground"]), dev(env, case["labels"]),
                                   dev(env, case["max_label"]), buf, ACC, model_method=model, angle_threshold=75, plane_seed=SEED,
                                   frame_ids=case["frame_ids"], nonuniform=nu)
    torch.cuda.synchronize()
    out = []
    for b in range(B):
        n = int(buf.nnz[b])
        d = dict(seg=buf.seg[b].cpu().numpy(), counts=buf.counts[b].cpu().numpy(), model=buf.model[b].cpu().numpy(), nnz=n,
                 q=buf.q16[b, :n].cpu().numpy(), q_row=buf.q16[b].cpu().numpy(), salience=None, key_point_map=None)
        if nu is not None:
            d.update(salience=buf.salience[b].cpu().numpy(), key_point_map=buf.key_point_map[b].cpu().numpy())
        out.append(d)
    return out, st.cpu().numpy()


def stage_reference(env, case, b, framework, model):
    """Frame b through the stage entries with ITS OWN M = max(max_label - 1, 1), as PointCloudSegment / QuantizationModule call them."""
    ops, cfg = env["ops"], env["cfg"]
    mx = int(case["max_label"][b])
    M = max(mx - 1, 1)
    ri, tm, ground = dev(env, case["ri"][b:b + 1]), dev(env, case["tm"]), dev(env, case["ground"][b:b + 1])
    seg = dev(env, case["labels"][b:b + 1].astype(np.uint16 if M > 254 else np.uint8))
    if model == "point":
        mod, counts = ops.point_model(ri, seg, ground, M)
    else:
        mod, counts = ops.plane_model(ri, tm, seg, M, angle_threshold=75, seed=SEED, ground=ground, want_counts=True, frame_ids=[int(case["frame_ids"][b])])
    sal = kp = lacc = None
    if framework == "nonuniform":
        _, kp = ops.extract_features(ri, seg, cfg["feature_region"], cfg["segments"], cfg["sharp_num"], cfg["less_sharp_num"], cfg["flat_num"])
        la = (np.array([ACC] * len(cfg["level_key_point_num"])) + np.array(cfg["level_delta_acc"])).astype(np.float32)
        sal, lacc = ops.salience(seg, kp, cfg["level_key_point_num"], la, cfg["ground_salience_level"], M)
    q, nnz, _ = ops.predict_quantize(ri, tm, seg, mod, ACC, M, int16=True, label_acc=lacc)
    n = int(nnz[0])
    return dict(seg=seg[0].cpu().numpy(), counts=counts[0].cpu().numpy(), model=mod[0].cpu().numpy(), nnz=n, q=q[0, :n].cpu().numpy(),
                salience=None if sal is None else sal[0].cpu().numpy(), key_point_map=None if kp is None else kp[0].cpu().numpy(), rows=mx + 1)


def assert_frame_equals_stages(got, ref, tag):
    r = ref["rows"]
    assert np.array_equal(got["seg"].astype(np.int64), ref["seg"].astype(np.int64)), tag
    assert np.array_equal(got["counts"][:r], ref["counts"][:r]) and not got["counts"][r:].any(), tag
    assert np.array_equal(bits(got["model"][:r]), bits(ref["model"][:r])), tag
    assert got["nnz"] == ref["nnz"] and np.array_equal(got["q"], ref["q"]), tag
    if ref["salience"] is not None:
        assert np.array_equal(got["salience"][:r], ref["salience"][:r]), tag
        assert np.array_equal(got["key_point_map"], ref["key_point_map"]), tag


def assert_frame_equals_oracle(env, case, b, got, tag):
    """Point model, uniform framework: oracle.point_modeling / intra_predict / uniform_quantize fed the same labels."""
    orc = env["orc"]
    ri, lab, tm = case["ri"][b], case["labels"][b], case["tm"]
    mp = orc.point_model_param(ri, lab, case["ground"][b])
    rows = mp.shape[0]                                         # max(seg) + 1
    assert np.array_equal(got["model"][:rows], mp.astype(np.float32), equal_nan=True), tag
    pred = orc.intra_predict(lab, mp, tm)
    q = orc.uniform_quantize(lab, ri.reshape(ri.shape + (1,)) - pred, ACC)
    assert got["nnz"] == q.shape[0] and np.array_equal(got["q"], q.astype(np.int16)), tag


# ---- 1. the entry against the stages it replaces ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", LC.CAPS)
@pytest.mark.parametrize("shape", LC.SHAPES)
def test_hand_made_maps_equal_the_stage_entries(env, shape, cap):
    for framework, model in COMBOS:
        # (the infinite and the NaN range: where the point model's sums leave their fixed-point window, with the uniform framework -- the
        # key-point kernel of the non-uniform one is specified for the projection's ranges, finite and >= 0)
        case = LC.batch(shape[0], shape[1], cap, nonfinite=(framework, model) == ("uniform", "point"))
        got, st = labels_call(env, case, framework, model, poison=0xAA)
        assert not st.any(), (framework, model, st)
        for b in range(3):
            tag = (shape, cap, framework, model, b)
            assert_frame_equals_stages(got[b], stage_reference(env, case, b, framework, model), tag)
            if (framework, model) == ("uniform", "point"):
                assert_frame_equals_oracle(env, case, b, got[b], tag)


def dbscan_case(env, shape):
    """B = 3: a blob image (tests/tile_cases.py's sweep clouds; on other shapes the same recipe) segmented by dbscan_segment at three
    (eps, min_points): three different max_label over one range image and ray table."""
    import tile_cases as TC
    H, W = shape
    seed = {(16, 128): 0, (64, 512): 2}.get(shape)
    if seed is not None:
        (ri, tm, ground), _ = TC.sweep_cloud(seed)
    else:
        rng = np.random.default_rng(H * W)
        n = H * W
        centres = rng.uniform(-20, 20, (12, 2))
        tm = np.zeros((n, 3), np.float32)
        tm[:, :2] = centres[rng.integers(0, 12, n)] + rng.normal(0, 0.8, (n, 2))
        ri = np.ones(n, np.float32)
        ri[rng.random(n) < 0.1] = 0.0
        tm[ri == 0] = (1.0, 0.0, 0.0)
        tm[(rng.random(n) < 0.1) & (ri != 0)] = (0.0, 0.0, -1.0)
        ri, tm, ground = ri.reshape(H, W), tm.reshape(H, W, 3), TC.GROUND.copy()
    labs, tops = [], []
    for eps, mp in ((0.2, 3), (0.9, 4), (3.0, 4)):      # (three different max_label on every shape: tests/dbscan_ref.py says so)
        seg, mx = env["db"].dbscan_segment(dev(env, ri[None]), dev(env, tm), dev(env, ground[None]), eps, min_points=mp)
        labs.append(seg[0].cpu().numpy()); tops.append(int(mx[0]))
    return dict(ri=np.stack([ri] * 3), tm=tm, ground=np.stack([ground] * 3), labels=np.stack(labs), max_label=np.array(tops, np.int32),
                frame_ids=np.array([3, 1, 2], np.int64))


@pytest.mark.parametrize("shape", LC.SHAPES)
def test_dbscan_labels_equal_the_stage_entries(env, shape):
    case = dbscan_case(env, shape)
    assert len(set(case["max_label"].tolist())) == 3 and case["max_label"].max() >= 4, case["max_label"]
    for cap in (LC.CAPS if case["max_label"].max() <= 255 else LC.CAPS[1:]):
        case["cap"] = cap
        for framework, model in COMBOS:
            got, st = labels_call(env, case, framework, model)
            assert not st.any()
            for b in range(3):
                assert_frame_equals_stages(got[b], stage_reference(env, case, b, framework, model), (shape, cap, framework, model, b))


def same_outputs(a, b, tag):
    for x, y in zip(a, b):
        for k in OUT_KEYS:
            assert (x[k] is None) == (y[k] is None)
            if x[k] is not None:
                assert np.array_equal(bits(np.asarray(x[k])), bits(np.asarray(y[k]))), (tag, k)


def test_workspace_may_hold_anything(env):
    """ws filled with 0xFF, and the same ws straight after a call of another shape, label type and model: the same results as from fresh buffers."""
    torch, lib = env["torch"], env["lib"]
    other = LC.batch(10, 70, 254)
    big = torch.empty(lib.lib().rpcc_labels_workspace_bytes(3, 16 * 128, 1022, 1) + 256, dtype=torch.uint8, device=env["dev"])
    for framework, model in (("uniform", "point"), ("nonuniform", "plane"), ("nonuniform", "point")):
        a = LC.batch(16, 128, 1022, nonfinite=(framework, model) == ("uniform", "point"))   # (the sums' flag must not survive in ws either)
        want, st = labels_call(env, a, framework, model)
        assert not st.any()
        big.fill_(0xFF)
        got, st = labels_call(env, a, framework, model, ws=big)
        assert not st.any()
        same_outputs(got, want, (framework, model, "0xFF"))
        labels_call(env, other, "nonuniform", "plane" if model == "point" else "point", ws=big)
        got, st = labels_call(env, a, framework, model, ws=big)
        assert not st.any()
        same_outputs(got, want, (framework, model, "after another shape"))


# ---- 2. refusals ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", LC.CAPS)
def test_refused_frames(env, cap):
    lib = env["lib"]
    for framework, model in (("uniform", "point"), ("nonuniform", "plane")):
        good = LC.batch(16, 128, cap)
        want, st = labels_call(env, good, framework, model)
        assert not st.any()
        for name, mx, plant, status in LC.refusals(cap):
            case = LC.batch(16, 128, cap)
            if mx is not None:
                case["max_label"][1] = mx
            else:
                (r, c), v = plant
                case["labels"][1, r, c] = v
                assert case["max_label"][1] <= cap + 1
            got, st = labels_call(env, case, framework, model, poison=0x5A)
            tag = (cap, framework, model, name)
            assert st.tolist() == [lib.LABELS_OK, getattr(lib, status), lib.LABELS_OK], tag
            bad = got[1]
            assert bad["nnz"] == 0, tag
            for k in ("seg", "counts", "model", "q_row", "salience", "key_point_map"):
                if bad[k] is not None:
                    assert not np.ascontiguousarray(bad[k]).view(np.uint8).any(), (tag, k)
            same_outputs([got[0], got[2]], [want[0], want[2]], tag)


# ---- 3. the front end against the per-frame tool ---------------------------------------------------------------------------------------------
def per_frame_blob(env, ds, xyz, fid, uniform, model, basic, ground=None):
    """tools/compress.py's stage sequence for one frame (segment_method DBSCAN, eps 1.5) -> the .rpcc bytes."""
    from rpcc_amd.segment_utils import PointCloudSegment
    from rpcc_amd.tools.compress import make_quantizer
    cu, cfg = env["cu"], env["cfg"]
    T = ds.PCTransformer
    ri = np.expand_dims(T.point_cloud_to_range_image(xyz), -1)
    pc = T.range_image_to_point_cloud(ri)
    cls = PointCloudSegment
    if ground is not None:
        class cls(PointCloudSegment):
            ransac_plane_segmentation = staticmethod(lambda pts, *a, **k: (None, ground))
    ps = cls(ds.transform_map, seed=SEED, frame_id=fid)
    seg_idx, gm = ps.segment(pc, ri, {"segment_method": "DBSCAN", "ground_vertical_threshold": 0.1, "cluster_num": 100, "DBSCAN_eps": 1.5})
    models = ps.cluster_modeling(pc, ri, seg_idx, {"model_method": model, "angle_threshold": cfg["plane_angle_threshold"]})
    model_param = np.concatenate((gm.reshape(1, 4), models), 0)
    residual = ri - ps.intra_predict(seg_idx, model_param)
    rq, sal, _ = make_quantizer(cfg, ACC, uniform).quantize_residual(residual, seg_idx, pc, ri)
    _, compressed = cu.compress_point_cloud(cu.BasicCompressor(method_name=basic), model_param, seg_idx, sal, rq, full=False)
    return cu.pack_bitstream(compressed, uniform=uniform), int(seg_idx.max())


def vlp16_frames(env):
    orc, synth = env["orc"], env["synth"]
    gd = orc.GEOMS["VelodyneVLP16"]
    fr = [synth.make_frame(100 + i, gd["H"], gd["W"], vmax_deg=gd["vmax_deg"], vmin_deg=gd["vmin_deg"]).numpy() for i in range(2)]
    rng = np.random.default_rng(5)      # an all-ground sweep: a disc on the plane z = -1.7
    r, a = rng.uniform(3.0, 40.0, 20000), rng.uniform(0, 2 * np.pi, 20000)
    fr.append(np.stack([r * np.cos(a), r * np.sin(a), np.full(r.size, -1.7)], 1).astype(np.float32))
    return fr, [101, 2002, 30003]


@pytest.fixture(scope="module")
def streams(env):
    """The per-frame containers every front-end test compares with: {(lidar, uniform, model, basic): (frames, ids, blobs)}."""
    cache = {}

    def get(lidar, uniform, model, basic):
        key = (lidar, uniform, model, basic)
        if key not in cache:
            ds = env["build_dataset"](lidar_type=lidar)
            if lidar == "Velodyne64E":
                frames, ids = [np.load(os.path.join(HERE, "golden", "example_64E.npz"))["xyz"]], [424242]
            else:
                frames, ids = vlp16_frames(env)
            cache[key] = (ds, frames, ids, [per_frame_blob(env, ds, f, i, uniform, model, basic)[0] for f, i in zip(frames, ids)])
        return cache[key]
    return get


def batch_compressor(env, ds, uniform, model, basic, **kw):
    return env["pl"].BatchCompressor(ds.PCTransformer, cluster_num=100, accuracy=ACC / 2, uniform=uniform, model_method=model, compressor_cfg=dict(env["cfg"]),
                                     basic_compressor=basic, seed=SEED, segment_method="DBSCAN", DBSCAN_eps=1.5, **kw)


@pytest.mark.parametrize("basic", ["bzip2", "lz4"])
@pytest.mark.parametrize("uniform,model", [(True, "point"), (False, "plane")])
def test_batch_compressor_equals_the_per_frame_tool(env, streams, uniform, model, basic):
    for lidar, caps in (("VelodyneVLP16", (None, 255)), ("Velodyne64E", (None,))):
        ds, frames, ids, want = streams(lidar, uniform, model, basic)
        for cap in caps:
            bc = batch_compressor(env, ds, uniform, model, basic, max_labels=cap)
            assert bc._buffers(len(frames)).seg.dtype == (env["torch"].uint8 if cap == 255 else env["torch"].uint16)
            got = bc.compress(frames, frame_ids=ids)
            assert got == want, (lidar, cap, [len(g) for g in got], [len(w) for w in want])


def test_a_frame_above_max_labels_is_named(env, streams):
    ds, frames, ids, want = streams("VelodyneVLP16", True, "point", "bzip2")
    many = LC.vlp16_many_clusters()
    _, top = per_frame_blob(env, ds, many, 9, True, "point", "bzip2", ground=LC.MANY_GROUND)
    assert top >= LC.MANY_MIN_LABEL
    grounds = np.tile(LC.MANY_GROUND, (3, 1))
    for basic in ("bzip2", "lz4"):
        bc = batch_compressor(env, ds, True, "point", basic, max_labels=40)
        with pytest.raises(env["lib"].RpccError, match=r"frames \[1\].*max_labels = 40"):
            bc.compress([frames[2], many, frames[2]], ground=grounds, frame_ids=[1, 9, 3])
        assert not any(b.in_flight for ring in bc._ring.values() for b in ring)       # the slot is free again
        assert len(bc.compress([frames[2]] * 3, ground=grounds, frame_ids=[1, 9, 3])) == 3
    # ... and under the default cap the same frame is what the per-frame tool writes
    bc = batch_compressor(env, ds, True, "point", "bzip2")
    blob, _ = per_frame_blob(env, ds, many, 9, True, "point", "bzip2", ground=LC.MANY_GROUND)
    assert bc.compress([many], ground=LC.MANY_GROUND[None], frame_ids=[9]) == [blob]


# ---- 4. streaming loader and tools ----------------------------------------------------------------------------------------------------------
def test_datalist_tools(env, streams, tmp_path):
    from rpcc_amd.tools import compress_datalist as cd, decompress_datalist as dd
    from rpcc_amd.tools.compress import make_parser
    from rpcc_amd.tools.decompress import decode_frame
    from rpcc_amd.utils import frame_identity
    cu = env["cu"]
    ds, frames, _, _ = streams("VelodyneVLP16", True, "point", "bzip2")
    src = tmp_path / "src"
    src.mkdir()
    names = []
    for i, f in enumerate(frames):
        names.append(str(src / ("%06d.bin" % i)))
        np.concatenate((f[:, :3], np.full((f.shape[0], 1), 0.5, np.float32)), 1).astype(np.float32).tofile(names[-1])
    (tmp_path / "list.txt").write_text("\n".join(names) + "\n")
    want = [per_frame_blob(env, ds, f, frame_identity(n), True, "point", "bzip2")[0] for f, n in zip(frames, names)]
    common = ["--lidar", "VelodyneVLP16", "--segment_method", "DBSCAN", "--DBSCAN_eps", "1.5", "--seed", str(SEED), "--accuracy", str(ACC / 2)]
    outs = {}
    for ingest in ("rows", "xyz"):
        out = tmp_path / ("out_" + ingest)
        cd.compress(make_parser(datalist=True).parse_args(["--datalist", str(tmp_path / "list.txt"), "--output_dir", str(out), "--batch", "2",
                                                           "--workers", "2", "--ingest", ingest] + common))
        outs[ingest] = [cd.output_path_for(str(out), n) for n in names]
        assert [open(p, "rb").read() for p in outs[ingest]] == want, ingest
    (tmp_path / "rpcc.txt").write_text("\n".join(outs["rows"]) + "\n")
    dec = tmp_path / "dec"
    a = make_parser(datalist=True).parse_args(["--datalist", str(tmp_path / "rpcc.txt"), "--output_dir", str(dec), "--batch_decode"] + common)
    dd.decompress(a)
    bz = cu.BasicCompressor(method_name="bzip2")
    for p in outs["rows"]:
        _, pc, _ = decode_frame(cu.read_compressed_bitstream(p, uniform=True), bz, ds.PCTransformer, None, ACC, None, True)
        ref = str(tmp_path / "ref.bin")
        ds.save_point_cloud_to_file(ref, pc.reshape(-1, 3))
        assert open(dd.output_path(a, p), "rb").read() == open(ref, "rb").read(), p


# ---- 5. decoder -----------------------------------------------------------------------------------------------------------------------------
def level_acc(env):
    return np.array([ACC] * len(env["cfg"]["level_key_point_num"])) + np.array(env["cfg"]["level_delta_acc"])


@pytest.mark.parametrize("uniform,model", [(True, "point"), (False, "plane")])
def test_batch_decompressor_equals_decode_frame(env, streams, uniform, model):
    from rpcc_amd.tools.decompress import decode_frame
    cu, pl = env["cu"], env["pl"]
    bz = cu.BasicCompressor(method_name="bzip2")
    lacc = level_acc(env)
    for lidar in ("VelodyneVLP16", "Velodyne64E"):
        ds, _, _, blobs = streams(lidar, uniform, model, "bzip2")
        T = ds.PCTransformer
        ref = [decode_frame(cu.unpack_bitstream(b, uniform=uniform), bz, T, None, ACC, lacc, uniform) for b in blobs]
        rows = [len(bz.decompress_dict(cu.unpack_bitstream(b, uniform=uniform))["plane_param"]) // 16 for b in blobs]
        for cap in (1023, max(rows) - 1):       # the second: the frame with the most rows goes through the per-frame fallback
            if cap < 2:
                continue
            got = pl.BatchDecompressor(T, None, ACC, uniform=uniform, level_acc=lacc, max_labels=cap).decompress(blobs)
            for (rec, pc, seg), (rrec, rpc, rseg) in zip(got, ref):
                assert np.array_equal(bits(rec), bits(rrec)) and np.array_equal(bits(pc), bits(rpc)), (lidar, cap)
                assert np.array_equal(seg.astype(np.int64), rseg.astype(np.int64)), (lidar, cap)
    with pytest.raises(ValueError, match="cluster_num=None"):
        pl.BatchDecompressor(T, None, ACC)


def test_long_salience_payload_is_refused_like_decode_frame(env, streams):
    """A non-uniform frame repacked with two extra salience bytes: rows < length <= cap + 2.  decode_frame(..., None, ...) sizes K from the rows
    and refuses it; so does the batch, by index and with the salience text."""
    from rpcc_amd.tools.decompress import decode_frame
    cu, pl = env["cu"], env["pl"]
    bz = cu.BasicCompressor(method_name="bzip2")
    lacc = level_acc(env)
    ds, _, _, blobs = streams("VelodyneVLP16", False, "plane", "bzip2")
    T = ds.PCTransformer
    d = bz.decompress_dict(cu.unpack_bitstream(blobs[1], uniform=False))
    rows = len(d["plane_param"]) // 16
    assert rows >= 3
    d = dict(d)
    d["salience_level"] = bytes(d["salience_level"]) + b"\x00\x00"
    assert rows < len(d["salience_level"]) <= 1022 + 2
    blob = cu.pack_bitstream(bz.compress_dict({k: np.frombuffer(bytes(v), np.uint8) for k, v in d.items()}), uniform=False)
    with pytest.raises(ValueError, match="salience_level holds more entries than labels"):
        decode_frame(cu.unpack_bitstream(blob, uniform=False), bz, T, None, ACC, lacc, False)
    bd = pl.BatchDecompressor(T, None, ACC, uniform=False, level_acc=lacc, max_labels=1023)
    status, seg, rec, pc = bd.decompress_device([blobs[0], blob, blobs[2]])
    assert status.cpu().tolist() == [0, env["lib"].STREAM_E_SALIENCE, 0]
    assert not seg[1].cpu().numpy().any() and not rec[1].cpu().numpy().view(np.uint32).any() and not pc[1].cpu().numpy().view(np.uint32).any()
    with pytest.raises(ValueError, match=r"frame 1: salience_level does not fit"):
        bd.decompress([blobs[0], blob, blobs[2]])
