"""-m gpu: stored rows (x, y, z, intensity), the non-uniform framework and the intensity trailer -- all six columns of the container schema --
through the three front ends that cut a batch's buffers into frames by compress_utils.frame_slices: the device containers, the host
assembly of BatchCompressor.collect and the streaming loader.  Three synthetic VLP-16 sweeps (16 x 1800), one byte string per frame."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ACC, GEOM, M, SCALE = 0.02, "VelodyneVLP16", 40, 100.0


def test_rows_nonuniform_intensity_through_all_three_front_ends():
    import torch
    assert torch.cuda.is_available()
    import __graft_entry__ as ge
    ge.build()
    from oracle import oracle as orc
    from rpcc_amd import compress_utils as cu
    from rpcc_amd import dataset, pipeline, synth
    from rpcc_amd.loader import StreamingCompressor
    gd = orc.GEOMS[GEOM]
    rng = np.random.default_rng(33)
    frames = []
    for i in range(3):
        xyz = synth.make_frame(8300 + i, gd["H"], gd["W"], vmax_deg=gd["vmax_deg"], vmin_deg=gd["vmin_deg"]).numpy()
        frames.append(np.ascontiguousarray(np.concatenate([xyz[:, :3], (rng.integers(0, 100, xyz.shape[0]) / np.float32(100))[:, None]], 1), dtype=np.float32))
    ids = [70, 71, 72]
    T = dataset.build_dataset(lidar_type=GEOM).PCTransformer
    mk = lambda method: pipeline.BatchCompressor(T, cluster_num=M, accuracy=ACC, uniform=False, basic_compressor=method, seed=4, intensity_scale=SCALE)
    # 1: the containers built on the device
    device = mk("rans").compress(frames, frame_ids=ids)
    # 2: the host assembly (bzip2 containers), every column re-coded as the per-frame path codes it
    rans, bz = cu.BasicCompressor(method_name="rans"), cu.BasicCompressor(method_name="bzip2")
    host = []
    for w in mk("bzip2").compress(frames, frame_ids=ids):
        cd = cu.unpack_bitstream(w, uniform=False, intensity=True)
        assert tuple(cd) == tuple(c.name for c in cu.columns(False, True))
        pay = np.frombuffer(bz.decompress(cd.pop("intensity")), np.uint8)
        rows = len(bz.decompress(cd["plane_param"])) // 16
        rq, idx_map, sal, plane = cu.decompress_point_cloud(cd, bz, rows, T.H, T.W)
        assert rq.size and sal.size == rows and pay.size > 8
        host.append(cu.pack_bitstream(cu.compress_point_cloud(rans, plane, idx_map, sal, rq, intensity=pay)[1], uniform=False))
    # 3: the streaming loader over the stored rows; the fourth slot of its batch is the empty pad frame
    got = {}
    assert StreamingCompressor(mk("rans"), batch=4, depth=2, workers=2, ingest="rows").run([(frames, ids)], sink=lambda k, blobs: got.update({k: blobs})) == 3
    assert len(device) == len(host) == len(got[0]) == 3 and len(set(device)) == 3
    for b in range(3):
        assert device[b] == host[b], b
        assert got[0][b] == device[b], b
