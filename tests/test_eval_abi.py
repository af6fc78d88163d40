"""librpcc_eval.so (include/rpcc_eval.h) builds, exports what its header declares and refuses bad arguments; the
numpy reference of the metrics agrees with an independent search.  No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    import rpcc_amd  # noqa: F401
    from rpcc_amd import _eval_lib
    return _eval_lib


def test_header_symbols_exported(built):
    hdr = open(os.path.join(ROOT, "include", "rpcc_eval.h")).read()
    declared = sorted(set(re.findall(r"\b(rpcc_[a-z0-9_]+)\s*\(", hdr)))
    assert len(declared) == 6
    lib = ctypes.CDLL(built.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    assert built.exported_symbols() == declared
    assert int(re.search(r"#define RPCC_EVAL_ABI_VERSION (\d+)", hdr).group(1)) == built.ABI_VERSION


def test_version_and_workspace(built):
    lib = built.lib()
    assert lib.rpcc_eval_version() == built.ABI_VERSION
    assert lib.rpcc_eval_workspace_bytes(64, 64, 2048) > 64 * 64 * 2048 * 16
    assert lib.rpcc_eval_workspace_bytes(0, 64, 2048) == 0
    assert lib.rpcc_eval_workspace_bytes(1, 1 << 14, 1 << 13) == 0   # above RPCC_EVAL_MAX_PIXELS


def test_argument_errors_do_not_crash(built):
    lib = built.lib()
    buf = ctypes.create_string_buffer(64)   # host memory: every call below must refuse before touching it
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.rpcc_eval_nn(p, p, 0, 64, 2048, 0, p, p, p, p, p, None, p, None) == -1
    assert b"bad argument" in lib.rpcc_eval_last_error()
    assert lib.rpcc_eval_nn(None, p, 1, 64, 2048, 0, p, p, p, p, p, None, p, None) == -1
    assert lib.rpcc_eval_nn(p, p, 1, 64, 2048, 6, p, p, p, p, p, None, p, None) == -1
    assert lib.rpcc_eval_normals(p, 1, 64, 2048, -1.0, 0, p, None, p, None) == -1
    assert lib.rpcc_eval_normals(p, 1, 0, 2048, 59.7, 0, p, None, p, None) == -1
    assert lib.rpcc_eval_metrics(p, p, 1, 64, 2048, p, None, None, 4e-4, p, p, None) == -1
    assert lib.rpcc_eval_metrics(p, p, 1, 64, 2048, p, p, None, -1.0, p, p, None) == -1
    assert b"bad argument" in lib.rpcc_eval_last_error()


def test_source_digest_unchanged_by_the_eval_library(built):
    from rpcc_amd import build as b
    before = b.source_digest()
    b.build_eval(force=True)
    assert b.source_digest() == before
    assert not any("csrc_eval" in d or d.endswith("rpcc_eval.h") for d in b.DEPS)
    assert os.path.exists(b.EVAL_LIB)
    tiles = os.path.join(os.path.dirname(b.__file__), "csrc_tile", "tiles.h")   # shared with the other side library
    assert tiles in b.EVAL_DEPS and tiles not in b.DEPS


def test_numpy_reference_search_is_exact():
    """eval_ref.nn / knn with a hint equal plain brute force, ties to the lowest index (duplicates, a grid of equal distances)."""
    import eval_ref as R
    rng = np.random.default_rng(5)
    s = np.round(rng.uniform(-3, 3, (700, 3)), 1).astype(np.float32)
    s[100:110] = s[5]                                   # duplicates
    q = np.round(rng.uniform(-3, 3, (300, 3)), 1).astype(np.float32)
    d, i = R.nn(q, s)
    D = R.d2(q, s)
    assert np.array_equal(d, D.min(1))
    for k in range(q.shape[0]):
        assert i[k] == np.nonzero(D[k] == D[k].min())[0][0]
    bad_hint = (i + 1) % s.shape[0]
    d2_, i2 = R.nn(q, s, hint=bad_hint)
    assert np.array_equal(d2_, d) and np.array_equal(i2, i)
    nb = R.knn(q, s, 1.0)
    nb2 = R.knn(q, s, 1.0, hint=np.tile(np.arange(12), (q.shape[0], 1)))
    assert np.array_equal(nb, nb2)
    for k in range(0, q.shape[0], 17):
        inr = np.nonzero(D[k] <= np.float32(1.0))[0]
        want = inr[np.argsort(D[k, inr], kind="stable")][:12]
        assert np.array_equal(nb[k, :len(want)], want) and np.all(nb[k, len(want):] == -1)


def test_numpy_reference_against_ckdtree():
    """Where scipy is installed, the reference's nearest distances agree with cKDTree (the reference's own PSNR search)."""
    spatial = pytest.importorskip("scipy.spatial")
    import eval_ref as R
    rng = np.random.default_rng(9)
    s = rng.uniform(-20, 20, (3000, 3)).astype(np.float32)
    q = (s[:2000] + rng.normal(0, 0.05, (2000, 3))).astype(np.float32)
    d, i = R.nn(q, s)
    dk, ik = spatial.cKDTree(s.astype(np.float64)).query(q.astype(np.float64))
    assert np.allclose(np.sqrt(d.astype(np.float64)), dk, rtol=1e-5, atol=1e-6)
    assert np.mean(i == ik) > 0.999
