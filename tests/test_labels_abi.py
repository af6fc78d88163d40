"""rpcc_compress_batch_labels without a GPU: the symbols and the interface version, the workspace size, the argument errors (raised before the
device is touched), the datalist tool's DBSCAN settings reaching the BatchCompressor it builds, and the claims of the hand-made label maps the
GPU tests use (tests/labels_cases.py)."""
import ctypes
import os

import numpy as np
import pytest

import labels_cases as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    import rpcc_amd  # noqa: F401
    from rpcc_amd import _lib
    return _lib


def test_symbols_and_version(built):
    lib = ctypes.CDLL(built.LIB_PATH)
    for name in ("rpcc_labels_workspace_bytes", "rpcc_compress_batch_labels"):
        assert hasattr(lib, name), name
        assert name in built.exported_symbols()
    assert built.lib().rpcc_version() == built.ABI_VERSION
    hdr = open(os.path.join(ROOT, "include", "rpcc_hip.h")).read()
    assert "#define RPCC_ABI_VERSION %d" % built.ABI_VERSION in hdr
    for name, val in (("RPCC_LABELS_OK", built.LABELS_OK), ("RPCC_LABELS_E_RANGE", built.LABELS_E_RANGE), ("RPCC_LABELS_E_CAPPED", built.LABELS_E_CAPPED)):
        assert "#define %s %d" % (name, val) in hdr
    from rpcc_amd import _seg_lib
    assert "#define RPCC_LABELS_CAPPED (%d)" % _seg_lib.CAPPED in hdr      # max_label as rpcc_seg_dbscan writes it


def test_workspace_size(built):
    lib = built.lib()
    P = 64 * 2048
    for M in (1, 100, 254, 255, built.MAX_CLUSTERS_MID):
        plain, general = lib.rpcc_labels_workspace_bytes(32, P, M, 0), lib.rpcc_labels_workspace_bytes(32, P, M, 1)
        assert 0 < plain < general
        assert plain >= lib.rpcc_codec_workspace_bytes(32, P, M) - 32 * 128 * 4      # the model part every stage carves from offset 0
        assert general >= lib.rpcc_plane_workspace_bytes(32, P, M)
    for B, P_, M in ((0, P, 100), (-1, P, 100), (3, 0, 100), (3, -5, 100), (3, P, 0), (3, P, -1), (3, P, built.MAX_CLUSTERS_MID + 1), (3, P, 65533)):
        assert lib.rpcc_labels_workspace_bytes(B, P_, M, 0) == 0 and lib.rpcc_labels_workspace_bytes(B, P_, M, 1) == 0, (B, P_, M)


def _io(built, p, **kw):
    f = dict(ri=p, tm=p, ground=p, labels=p, max_label=p, frame_ids=None, seg=p, model=p, counts=p, q16=p, nnz=p, status=p, model_method=0,
             plane_cos_cut=0.0, plane_seed=0, nonuniform=None, salience=None, key_point_map=None)
    f.update(kw)
    return built.LabelsIO(**f)


def test_argument_errors_before_the_device(built):
    """Every pointer is a host dummy that must never reach a kernel: the call returns RPCC_ERR_ARG first."""
    lib = built.lib()
    dummy = ctypes.create_string_buffer(256)
    p = ctypes.addressof(dummy)
    geom = built.Geom(16, 128, 6.2831855, 0.26, -0.26)

    def call(io, B=3, M=100, ws=p, g=geom):
        return lib.rpcc_compress_batch_labels(ctypes.byref(io) if io is not None else None, B, g, M, 0.04, ws, None)

    assert call(None) == -1 and b"bad argument" in lib.rpcc_last_error()
    assert call(_io(built, p), ws=None) == -1
    for name in ("ri", "tm", "ground", "labels", "max_label", "seg", "model", "counts", "q16", "nnz", "status"):
        assert call(_io(built, p, **{name: None})) == -1, name
        assert b"bad argument" in lib.rpcc_last_error()
    for M in (0, -3, built.MAX_CLUSTERS_MID + 1, 65533):
        assert call(_io(built, p), M=M) == -1, M
    for B in (0, -1, 65536):
        assert call(_io(built, p), B=B) == -1, B
    for mm in (-1, 2, 7):
        assert call(_io(built, p, model_method=mm)) == -1 and b"model_method" in lib.rpcc_last_error(), mm
    nu = built.NonuniformCfg()
    nu.levels, nu.ground_level = 4, 2
    assert call(_io(built, p, nonuniform=ctypes.addressof(nu))) == -1          # no salience / key_point_map
    nu.levels = 9
    assert call(_io(built, p, nonuniform=ctypes.addressof(nu), salience=p, key_point_map=p)) == -1
    assert call(_io(built, p), g=built.Geom(1, 128, 6.28, 0.26, -0.26)) == -1


class _Stub:
    """Stands in for loader.StreamingCompressor: keeps the BatchCompressor the datalist driver built."""
    seen = []

    def __init__(self, bc, batch, depth, workers, pool, points_per_frame, ingest):
        _Stub.seen.append(bc)
        self.B = batch

    def run(self, batches, sink, entropy=True):
        n = 0
        for k, (frames, fids) in enumerate(batches):
            sink(k, [b"x" for _ in frames])
            n += len(frames)
        return n


def _run_datalist(tmp_path, extra):
    import rpcc_amd  # noqa: F401
    from rpcc_amd.tools import compress_datalist as cd
    from rpcc_amd.tools.compress import make_parser
    names = ["/data/seq00/%06d.bin" % i for i in range(3)]
    (tmp_path / "list.txt").write_text("\n".join(names) + "\n")
    out = tmp_path / "out"
    a = make_parser(datalist=True).parse_args(["--datalist", str(tmp_path / "list.txt"), "--output_dir", str(out), "--lidar", "VelodyneVLP16"] + extra)
    _Stub.seen.clear()
    cd.compress(a, streaming_factory=_Stub)
    (bc,) = _Stub.seen
    return bc


def test_datalist_settings_reach_the_batch_compressor(built, tmp_path):
    bc = _run_datalist(tmp_path, ["--segment_method", "DBSCAN", "--DBSCAN_eps", "0.9", "--max_labels", "300"])
    assert bc.segment_method == "DBSCAN" and bc.dbscan and bc.eps == 0.9 and bc.M == 299
    bc = _run_datalist(tmp_path, ["--segment_method", "DBSCAN"])
    assert bc.dbscan and bc.M == built.MAX_CLUSTERS_MID        # labels up to 1023: where the per-frame path raises
    from rpcc_amd.utils import load_compressor_cfg
    from rpcc_amd.tools.compress import PKG
    cfg = load_compressor_cfg(os.path.join(PKG, "cfgs/compressor.yaml"))
    bc = _run_datalist(tmp_path, [])
    assert bc.segment_method == cfg["segment_method"] == "FPS" and not bc.dbscan and bc.M == cfg["cluster_num"]


def test_constructor_limits(built):
    import rpcc_amd  # noqa: F401
    from rpcc_amd.dataset import build_dataset
    from rpcc_amd.pipeline import BatchCompressor, BatchDecompressor, MixedBatchCompressor
    T = build_dataset(lidar_type="VelodyneVLP16").PCTransformer
    assert BatchCompressor(T, cluster_num=7, segment_method="DBSCAN", max_labels=255).M == 254        # cluster_num is ignored
    for bad in (1, 1024, 70000):
        with pytest.raises(built.RpccError, match="max_labels"):
            BatchCompressor(T, segment_method="DBSCAN", max_labels=bad)
    with pytest.raises(ValueError):
        BatchCompressor(T, segment_method="KMEANS")
    with pytest.raises(NotImplementedError, match="DBSCAN"):
        MixedBatchCompressor({"VelodyneVLP16": T}, segment_method="DBSCAN")
    with pytest.raises(ValueError, match="cluster_num=None"):
        BatchDecompressor(T, None, 0.04)
    bd = BatchDecompressor(T, None, 0.04, max_labels=1023)
    assert bd.M == 1022 and bd.cluster_num is None and bd.per_frame_rows
    assert BatchDecompressor(T, 100, 0.04).cluster_num == 100


@pytest.mark.parametrize("cap", LC.CAPS)
@pytest.mark.parametrize("shape", LC.SHAPES)
def test_case_builders_hold_their_claims(shape, cap):
    for nonfinite in (False, True):
        b = LC.batch(shape[0], shape[1], cap, nonfinite=nonfinite)
        assert b["labels"].shape == (3,) + shape and len(set(b["max_label"].tolist())) == 3
        for i in range(3):
            LC.check_frame(b["ri"][i], b["labels"][i], b["facts"][i], cap)
            assert b["facts"][i]["max_label"] == b["max_label"][i]
        f0, f1, f2 = b["facts"]
        assert f0["max_label"] == cap + 1 and f0["used"][-1] == cap + 1 and f0["empty_labels"]       # reaches M + 1; unused labels below it
        assert f2["used"][-1] < f2["max_label"]                                                       # the top label is empty
        assert (f1["max_label"], f1["used"]) in ((2, [0, 1, 2]), (0, [0]))
        assert bool(f2["nonfinite"]) == nonfinite
        if cap > 254:
            assert max(f0["used"]) >= 256 and max(f2["used"]) >= 256
    for name, mx, plant, status in LC.refusals(cap):
        assert (mx is None) != (plant is None)
        if mx is not None:
            assert mx == -1 or mx < -1 or mx > cap + 1
        else:
            assert plant[1] < 0 or plant[1] > cap + 1


def test_many_cluster_frame_exceeds_a_small_cap():
    import dbscan_ref as R
    from oracle import oracle as orc
    g = orc.LidarGeom(**orc.GEOMS["VelodyneVLP16"])
    ri = orc.project(LC.vlp16_many_clusters(), g)
    seg = R.dbscan_frame(ri, orc.transform_map(g), LC.MANY_GROUND, 1.5)
    assert LC.MANY_MIN_LABEL <= seg.max() <= 254
    assert not (seg == 3).any() and (seg == 1).any()     # the origin cluster (label 3) holds only zero-range pixels, which all became label 1
