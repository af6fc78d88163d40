"""DBSCAN segmentation on the MI355X (rpcc_amd.dbscan, librpcc_seg.so) against the numpy reference (tests/dbscan_ref.py)
and the sklearn golden of the real sweep: the hand fixtures, pruned = brute force bit for bit, batches, the stage
limit, the end-to-end round trip and the compress tool."""
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
    import dbscan_ref
    from rpcc_amd import dbscan, synth
    from oracle import oracle as orc
    assert torch.cuda.is_available()
    return dict(torch=torch, R=dbscan_ref, db=dbscan, synth=synth, orc=orc, dev=torch.device("cuda:0"))


def run(env, ri, tm, ground, eps=1.5, min_points=10, brute=False, stats=False):
    """numpy ri [B,H,W] (or [H,W]), tm [H,W,3], ground [B,4] (or [4]) -> numpy (seg, max_label[, stats])."""
    torch, dev = env["torch"], env["dev"]
    ri = np.asarray(ri, np.float32)
    ri = ri[None] if ri.ndim == 2 else ri
    ground = np.asarray(ground, np.float64).reshape(-1, 4)
    out = env["db"].dbscan_segment(torch.from_numpy(np.ascontiguousarray(ri)).to(dev), torch.from_numpy(np.ascontiguousarray(tm)).to(dev),
                                   torch.from_numpy(ground).to(dev), eps, min_points, brute_force=brute, stats=stats)
    return tuple(o.cpu().numpy() for o in out)


def golden(env, case, geom):
    orc = env["orc"]
    z = np.load(os.path.join(HERE, "golden", case + ".npz"))
    g = orc.LidarGeom(**orc.GEOMS[geom])
    return orc.project(z["xyz"], g), orc.transform_map(g), z["ground_model"]


def full_frames(env):
    """64 x 2048 frames: the default scene and the adversarial scenes of the FPS study, and one with no zero-range pixel."""
    orc, synth = env["orc"], env["synth"]
    gd = orc.GEOMS["Velodyne64E_2048"]
    g = orc.LidarGeom(**gd)
    tm = orc.transform_map(g)
    ris = []
    for fid, scene in ((1, "default"), (2, "noise"), (3, "shell"), (4, "corridor")):
        f = synth.make_frame(fid, gd["H"], gd["W"], vmax_deg=gd["vmax_deg"], vmin_deg=gd["vmin_deg"], scene=scene).numpy()
        ris.append(orc.project(f, g))
    filled = ris[0].copy()
    filled[filled == 0] = 60.0
    ris.append(filled)
    gm = np.load(os.path.join(HERE, "golden", "synth_64x2048.npz"))["ground_model"]
    return np.stack(ris), tm, np.tile(gm, (len(ris), 1))


@pytest.mark.parametrize("name", ["boundary_strict", "boundary_inside", "min_points_self", "border_lowest", "origin_keeps_number",
                                  "ground_noise"])
def test_hand_fixtures(env, name):
    R = env["R"]
    ri, tm, mp, want = R.fixtures()[name]
    ref = R.dbscan_frame(ri, tm, R.GROUND, 1.5, mp)
    for brute in (False, True):
        seg, mx = run(env, ri, tm, R.GROUND, 1.5, mp, brute=brute)
        assert np.array_equal(seg[0], ref), (name, brute)
        assert seg[0].reshape(-1)[:len(want)].tolist() == want
        assert mx[0] == ref.max()


def test_synth_vlp16_equals_reference(env):
    R = env["R"]
    ri, tm, gm = golden(env, "synth_vlp16", "VelodyneVLP16")
    seg, mx = run(env, ri, tm, gm)
    ref = R.dbscan_frame(ri, tm, gm, 1.5)
    assert np.array_equal(seg[0], ref)
    assert mx[0] == ref.max()


def test_example_64E_equals_golden(env):
    ri, tm, gm = golden(env, "example_64E", "Velodyne64E")
    gold = np.load(os.path.join(HERE, "golden", "dbscan_example_64E.npz"))["seg_idx"]
    seg, mx = run(env, ri, tm, gm)
    assert np.array_equal(seg[0], gold.astype(np.int32))
    assert mx[0] == gold.max()


def test_pruned_equals_bruteforce_fullsize(env):
    """Pruned and brute force bit for bit, frame by frame and as a batch; a repeat run is identical; pruning tests fewer pairs."""
    ris, tm, gms = full_frames(env)
    seg, mx, st = run(env, ris, tm, gms, stats=True)
    bseg, bmx, bst = run(env, ris, tm, gms, brute=True, stats=True)
    assert np.array_equal(seg, bseg) and np.array_equal(mx, bmx)
    assert np.all(st[:, 0] < bst[:, 0])
    seg2, mx2 = run(env, ris, tm, gms)
    assert np.array_equal(seg, seg2) and np.array_equal(mx, mx2)
    for b in range(ris.shape[0]):
        s1, m1 = run(env, ris[b], tm, gms[b])
        assert np.array_equal(s1[0], seg[b]) and m1[0] == mx[b], b
    assert (ris[4] != 0).all() and not (seg[4] == 1).any()
    assert mx.max() >= 4   # not a trivial batch: some frame holds clusters


def test_mixed_batch_equals_single_frames(env):
    """Frames of different content in one call (a VLP-16 sweep in a 64-row image would not fit: use three scenes of one
    geometry and a frame of hand fixtures padded into it) give what each gives alone."""
    R = env["R"]
    ris, tm, gms = full_frames(env)
    fri, ftm, _, _ = R.fixtures()["border_lowest"]
    mixed = np.stack([ris[2], ris[0], ris[3]])
    seg, mx = run(env, mixed, tm, gms[:3])
    for b in range(3):
        s1, m1 = run(env, mixed[b], tm, gms[b])
        assert np.array_equal(s1[0], seg[b]) and m1[0] == mx[b]
    seg_f, _ = run(env, np.stack([fri, fri]), ftm, np.stack([R.GROUND, R.GROUND]), 1.5, 4)
    assert np.array_equal(seg_f[0], seg_f[1]) and np.array_equal(seg_f[0], R.dbscan_frame(fri, ftm, R.GROUND, 1.5, 4))


def test_too_many_clusters_raise(env):
    """More clusters than the stage entries take: PointCloudSegment names RPCC_MAX_CLUSTERS_MID instead of truncating."""
    from rpcc_amd._lib import RpccError
    from rpcc_amd.segment_utils import PointCloudSegment
    R = env["R"]
    entries = []
    for k in range(1030):
        entries += [("p", (float(k % 40) * 4.0, float(k // 40) * 4.0, 0.0))] * 10
    ri, tm = R.frame(entries, 64, 256)
    seg, mx = run(env, ri, tm, R.GROUND)
    assert mx[0] == 1030 + 2

    class Seg(PointCloudSegment):
        ransac_plane_segmentation = staticmethod(lambda pts, *a, **k: (None, R.GROUND))

    ps = Seg(tm)
    cfg = {"segment_method": "DBSCAN", "ground_vertical_threshold": 0.1, "cluster_num": 100, "DBSCAN_eps": 1.5}
    with pytest.raises(RpccError, match="RPCC_MAX_CLUSTERS_MID"):
        ps.segment(R.points(ri, tm), ri[..., None], cfg)


@pytest.mark.parametrize("uniform", [True, False])
def test_end_to_end_roundtrip(env, uniform):
    """PointCloudSegment (DBSCAN, golden ground injected) -> point model -> prediction -> quantisation -> container ->
    decode_frame: the labels come back and the depth error stays within the accuracy."""
    from rpcc_amd import compress_utils as cu
    from rpcc_amd.dataset import build_dataset
    from rpcc_amd.segment_utils import PointCloudSegment
    from rpcc_amd.tools.decompress import decode_frame, stream_cluster_num
    z = np.load(os.path.join(HERE, "golden", "example_64E.npz"))
    gold = np.load(os.path.join(HERE, "golden", "dbscan_example_64E.npz"))["seg_idx"]
    ds = build_dataset(lidar_type="Velodyne64E")
    T = ds.PCTransformer
    ri = np.expand_dims(T.point_cloud_to_range_image(z["xyz"]), -1)
    pc = T.range_image_to_point_cloud(ri)
    gm = z["ground_model"]

    class Seg(PointCloudSegment):
        ransac_plane_segmentation = staticmethod(lambda pts, *a, **k: (None, gm))

    cfg = {"segment_method": "DBSCAN", "ground_vertical_threshold": 0.1, "cluster_num": 100, "DBSCAN_eps": 1.5}
    ps = Seg(ds.transform_map)
    seg_idx, ground_model = ps.segment(pc, ri, cfg)
    assert seg_idx.dtype == np.int64 and np.array_equal(seg_idx, gold)
    models = ps.cluster_modeling(pc, ri, seg_idx, {"model_method": "point", "angle_threshold": 75})
    model_param = np.concatenate((ground_model.reshape(1, 4), models), 0)
    assert model_param.shape[0] == seg_idx.max() + 1
    residual = ri - ps.intra_predict(seg_idx, model_param)
    accuracy = 0.04
    if uniform:
        QM = cu.QuantizationModule(accuracy)
    else:
        QM = cu.QuantizationModule(accuracy, uniform=False)
    rq, sal, _ = QM.quantize_residual(residual, seg_idx, pc, ri)
    bc = cu.BasicCompressor(method_name="bzip2")
    _, compressed = cu.compress_point_cloud(bc, model_param, seg_idx, sal, rq, full=False)
    blob = cu.unpack_bitstream(cu.pack_bitstream(compressed, uniform=uniform), uniform=uniform)
    lacc = np.array([accuracy] * 4) + np.array([0, 0.02, 0.04, 0.06])
    rec, _, seg_rec = decode_frame(blob, bc, T, stream_cluster_num(cfg), accuracy, lacc, uniform, want_points=False)
    assert np.array_equal(seg_rec.astype(np.int64), seg_idx)
    err = np.abs(rec - ri[..., 0])
    assert err.max() <= accuracy / 2 + (0.0 if uniform else 0.06) + 1e-5


def test_compress_tool_dbscan_eval(env, tmp_path, capsys):
    """tools/compress.py --segment_method DBSCAN --eval on the real sweep prints the reference's lines."""
    from rpcc_amd.tools import compress as tc
    z = np.load(os.path.join(HERE, "golden", "example_64E.npz"))
    src = tmp_path / "frame.bin"
    np.concatenate((z["xyz"], np.zeros((z["xyz"].shape[0], 1), np.float32)), 1).astype(np.float32).tofile(src)
    out = tmp_path / "frame_dbscan.bin"
    capsys.readouterr()
    tc.compress(tc.make_parser().parse_args(["--input", str(src), "--output", str(out), "--eval", "--lidar", "Velodyne64E",
                                             "--segment_method", "DBSCAN", "--DBSCAN_eps", "1.5", "--cluster_num", "400"]))
    text = capsys.readouterr().out
    assert os.path.getsize(out) > 0
    for label in ("Compression finished.", "    Segmentation module: ", "    BPP: ", "    Depth Error (max): ", "    Chamfer Distance (mean): ",
                  "    F1 score (threshold=0.02): ", "    Point-to-Point PSNR (r=59.7): ", "    Point-to-Plane PSNR (r=59.7): "):
        assert sum(1 for ln in text.splitlines() if ln.startswith(label)) == 1, label
    assert "batch front-end" not in text
