"""librpcc_seg.so (include/rpcc_seg.h) builds, exports what its header declares and refuses bad arguments; the numpy
DBSCAN reference (tests/dbscan_ref.py) pins every rule of DESIGN.md section 10 and agrees with sklearn.  No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    import rpcc_amd  # noqa: F401
    from rpcc_amd import _seg_lib
    return _seg_lib


def test_header_symbols_exported(built):
    hdr = open(os.path.join(ROOT, "include", "rpcc_seg.h")).read()
    declared = sorted(set(re.findall(r"\b(rpcc_[a-z0-9_]+)\s*\(", hdr)))
    assert len(declared) == 4
    lib = ctypes.CDLL(built.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    assert built.exported_symbols() == declared
    assert int(re.search(r"#define RPCC_SEG_ABI_VERSION (\d+)", hdr).group(1)) == built.ABI_VERSION
    for name, val in (("RPCC_SEG_BRUTEFORCE", built.BRUTEFORCE), ("RPCC_SEG_NSTATS", built.NSTATS), ("RPCC_SEG_CAPPED", built.CAPPED)):
        assert int(re.search(r"#define %s \(?(-?\d+)\)?" % name, hdr).group(1)) == val, name


def test_version_and_workspace(built):
    lib = built.lib()
    assert lib.rpcc_seg_version() == built.ABI_VERSION
    assert lib.rpcc_seg_workspace_bytes(32, 64, 2048) >= 32 * 64 * 2048 * 24
    assert lib.rpcc_seg_workspace_bytes(1, 1, 1) > 0
    assert lib.rpcc_seg_workspace_bytes(0, 64, 2048) == 0
    assert lib.rpcc_seg_workspace_bytes(1, 0, 2048) == 0
    assert lib.rpcc_seg_workspace_bytes(65536, 1, 1) == 0
    assert lib.rpcc_seg_workspace_bytes(1, 1 << 14, 1 << 13) == 0   # above RPCC_SEG_MAX_PIXELS


def test_argument_errors_do_not_crash(built):
    lib = built.lib()
    buf = ctypes.create_string_buffer(64)   # host memory: every call below must refuse before touching it
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.rpcc_seg_dbscan(p, p, p, 0, 64, 2048, 1.5, 10, 0, p, p, None, p, None) == -1
    assert b"bad argument" in lib.rpcc_seg_last_error()
    assert lib.rpcc_seg_dbscan(None, p, p, 1, 64, 2048, 1.5, 10, 0, p, p, None, p, None) == -1
    assert lib.rpcc_seg_dbscan(p, p, p, 1, 64, 2048, 1.5, 10, 0, p, None, None, p, None) == -1
    assert lib.rpcc_seg_dbscan(p, p, p, 1, 64, 2048, 1.5, 10, 0, p, p, None, None, None) == -1
    assert lib.rpcc_seg_dbscan(p, p, p, 1, 64, 2048, -1.5, 10, 0, p, p, None, p, None) == -1
    assert lib.rpcc_seg_dbscan(p, p, p, 1, 64, 2048, float("nan"), 10, 0, p, p, None, p, None) == -1
    assert lib.rpcc_seg_dbscan(p, p, p, 1, 64, 2048, 1e20, 10, 0, p, p, None, p, None) == -1
    assert lib.rpcc_seg_dbscan(p, p, p, 1, 64, 2048, 1.5, 0, 0, p, p, None, p, None) == -1
    assert lib.rpcc_seg_dbscan(p, p, p, 1, 64, 2048, 1.5, 10, 2, p, p, None, p, None) == -1
    assert b"bad argument" in lib.rpcc_seg_last_error()


def test_source_digest_unchanged_by_the_seg_library(built):
    from rpcc_amd import build as b
    before = b.source_digest()
    b.build_seg(force=True)
    assert b.source_digest() == before
    assert not any("csrc_seg" in d or d.endswith("rpcc_seg.h") for d in b.DEPS)
    assert os.path.exists(b.SEG_LIB)
    tiles = os.path.join(os.path.dirname(b.__file__), "csrc_tile", "tiles.h")   # shared with the other side library
    assert tiles in b.SEG_DEPS and tiles not in b.DEPS


@pytest.mark.parametrize("name", ["boundary_strict", "boundary_inside", "min_points_self", "border_lowest", "origin_keeps_number",
                                  "ground_noise"])
def test_reference_pins_each_rule(name):
    """d^2 == eps^2 is not a neighbour; min_points counts the point itself; a border point takes the lower cluster number;
    the origin cluster keeps its number while its pixels become 1; noise 2, ground 0."""
    import dbscan_ref as R
    ri, tm, mp, want = R.fixtures()[name]
    seg = R.dbscan_frame(ri, tm, R.GROUND, 1.5, mp).reshape(-1)
    assert seg[:len(want)].tolist() == want
    assert not seg[len(want):].any()


def test_reference_on_real_sweep_matches_golden_head():
    """The golden of the real sweep (sklearn) and the reference agree on the labels of the first rows (cheap: the full frame
    is the GPU test's job) -- here only the mask and the ri == 0 rule, which need no search."""
    import dbscan_ref as R
    from oracle import oracle as orc
    z = np.load(os.path.join(HERE, "golden", "example_64E.npz"))
    gold = np.load(os.path.join(HERE, "golden", "dbscan_example_64E.npz"))["seg_idx"]
    g = orc.LidarGeom(**orc.GEOMS["Velodyne64E"])
    ri = orc.project(z["xyz"], g)
    ng = R.nonground(ri, orc.transform_map(g), z["ground_model"])
    assert np.array_equal(gold == 0, ~ng & (ri != 0))
    assert np.array_equal(gold == 1, ri == 0)
    assert int(ng.sum()) == 95164 and int((ng & (ri == 0)).sum()) == 33947


def test_reference_against_sklearn_synth_vlp16():
    pytest.importorskip("sklearn")
    import dbscan_ref as R
    from oracle import oracle as orc
    z = np.load(os.path.join(HERE, "golden", "synth_vlp16.npz"))
    g = orc.LidarGeom(**orc.GEOMS["VelodyneVLP16"])
    tm = orc.transform_map(g)
    ri = orc.project(z["xyz"], g)
    assert np.array_equal(R.dbscan_frame(ri, tm, z["ground_model"], 1.5), R.sklearn_labels(ri, tm, z["ground_model"], 1.5))


@pytest.mark.parametrize("seed", range(4))
def test_reference_against_sklearn_random(seed):
    """Random clouds in blobs plus zero-range pixels; the coordinates are multiples of 2^-7 away from 1.5-multiples by a random
    offset, and pairs at exactly d^2 == 2.25 are ruled out before comparing (sklearn counts d <= eps)."""
    pytest.importorskip("sklearn")
    import dbscan_ref as R
    rng = np.random.default_rng(seed)
    H, W = 16, 128
    n = H * W
    centres = rng.uniform(-20, 20, (12, 2))
    xy = centres[rng.integers(0, 12, n)] + rng.normal(0, rng.uniform(0.3, 1.5), (n, 2))
    tm = np.zeros((n, 3), np.float32)
    tm[:, :2] = xy
    ri = np.ones(n, np.float32)
    ri[rng.random(n) < 0.1] = 0.0
    tm[ri == 0] = (1.0, 0.0, 0.0)
    ground_pix = rng.random(n) < 0.1
    tm[ground_pix & (ri != 0)] = (0.0, 0.0, -1.0)
    ri, tm = ri.reshape(H, W), tm.reshape(H, W, 3)
    pts = R.points(ri, tm)[R.nonground(ri, tm, R.GROUND)].astype(np.float64)
    assert not np.any(R.d2(pts[:, None], pts[None]) == 2.25)
    mp = int(rng.integers(3, 12))
    assert np.array_equal(R.dbscan_frame(ri, tm, R.GROUND, 1.5, mp), R.sklearn_labels(ri, tm, R.GROUND, 1.5, mp))
