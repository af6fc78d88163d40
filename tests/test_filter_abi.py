"""librpcc_filter.so (include/rpcc_filter.h) builds, exports what its header declares and refuses bad arguments.  No GPU needed."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    import rpcc_amd  # noqa: F401
    from rpcc_amd import _filter_lib
    return _filter_lib


def test_header_symbols_exported(built):
    hdr = open(os.path.join(ROOT, "include", "rpcc_filter.h")).read()
    declared = sorted(set(re.findall(r"\b(rpcc_[a-z0-9_]+)\s*\(", hdr)))
    assert len(declared) == 4
    lib = ctypes.CDLL(built.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    assert built.exported_symbols() == declared
    assert int(re.search(r"#define RPCC_FILTER_ABI_VERSION (\d+)", hdr).group(1)) == built.ABI_VERSION == 1
    for name, val in (("RPCC_FILTER_BRUTEFORCE", built.BRUTEFORCE), ("RPCC_FILTER_NSTATS", built.NSTATS), ("RPCC_FILTER_TILE", built.TILE),
                      ("RPCC_FILTER_TILE_LIST", built.TILE_LIST)):
        assert int(re.search(r"#define %s \(?(-?\d+)\)?" % name, hdr).group(1)) == val, name
    import filter_cases as FC
    assert (FC.TILE, FC.TILE_LIST) == (built.TILE, built.TILE_LIST)


def test_version_and_workspace(built):
    lib = built.lib()
    assert lib.rpcc_filter_version() == built.ABI_VERSION
    nt = 122320 // 256 + 1
    assert lib.rpcc_filter_workspace_bytes(122320, 1) >= nt * 36 + 8
    assert lib.rpcc_filter_workspace_bytes(0, 1) > 0
    assert lib.rpcc_filter_workspace_bytes(32 * 122320, 32) < 32 * 122320      # a fraction of the points' own bytes
    assert lib.rpcc_filter_workspace_bytes(1000, 0) == 0
    assert lib.rpcc_filter_workspace_bytes(1000, -1) == 0
    assert lib.rpcc_filter_workspace_bytes(-1, 1) == 0
    assert lib.rpcc_filter_workspace_bytes(1000, 65536) == 0
    assert lib.rpcc_filter_workspace_bytes(1000, 65535) > 0
    assert lib.rpcc_filter_workspace_bytes((1 << 30) + 1, 1) == 0      # above RPCC_FILTER_MAX_POINTS


def test_argument_errors_do_not_crash(built):
    lib = built.lib()
    buf = ctypes.create_string_buffer(64)   # host memory: every call below must refuse before touching it
    p = ctypes.cast(buf, ctypes.c_void_p)
    q = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    call = lambda points=p, stride=12, offsets=p, total=4, B=1, radius=1.0, nb=3, flags=0, keep=p, masked=None, ws=p: \
        lib.rpcc_filter_radius(points, stride, offsets, total, B, radius, nb, flags, keep, None, None, masked, None, ws, None)
    assert call(B=0) == -1
    assert b"bad argument" in lib.rpcc_filter_last_error()
    for bad in (dict(B=65536), dict(total=-1), dict(total=(1 << 30) + 1), dict(points=None), dict(offsets=None), dict(keep=None), dict(ws=None),
                dict(radius=0.0), dict(radius=-1.0), dict(radius=float("nan")), dict(radius=1e20), dict(radius=1e-20), dict(nb=-1),
                dict(flags=2), dict(flags=-1), dict(stride=8), dict(stride=4), dict(stride=20), dict(masked=p)):
        assert call(**bad) == -1, bad
        assert b"bad argument" in lib.rpcc_filter_last_error(), bad
    assert call(masked=q, B=0) == -1
    assert buf.raw == b"\0" * 64


def test_source_digest_unchanged_by_the_filter_library(built):
    from rpcc_amd import build as b
    before = b.source_digest()
    b.build_filter(force=True)
    assert b.source_digest() == before
    assert not any("csrc_filter" in d or d.endswith("rpcc_filter.h") for d in b.DEPS)
    assert os.path.exists(b.FILTER_LIB)
    tiles = os.path.join(os.path.dirname(b.__file__), "csrc_tile", "tiles.h")   # shared with the other side libraries
    assert tiles in b.FILTER_DEPS and tiles not in b.DEPS
    assert not any("csrc_seg" in d for d in b.FILTER_DEPS)


def test_front_ends_name_the_missing_gpu(built):
    """Without a visible GPU remove_radius_outlier -- and with it DatasetTemplate.__getitem__ under use_radius_outlier_removal -- raises
    RpccError by name; nothing falls back to the CPU.  (With one, the same call answers.)"""
    import numpy as np
    import torch
    from rpcc_amd._lib import RpccError
    from rpcc_amd.outlier import remove_radius_outlier
    pts = np.zeros((5, 3), np.float64)
    if torch.cuda.is_available():
        filtered, index = remove_radius_outlier(pts)
        assert filtered.shape == (5, 3) and index.tolist() == [0, 1, 2, 3, 4]
    else:
        with pytest.raises(RpccError, match="needs a GPU"):
            remove_radius_outlier(pts)
