"""librpcc_deflate.so (include/rpcc_deflate.h) builds, exports what its header declares, reports its version and bound, and
refuses bad arguments before touching memory; csrc/, build.DEPS and source_digest() do not change with it or with the match
finder it shares with librpcc_lz4.so.  No GPU needed."""
import ctypes
import gzip
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
    from rpcc_amd import _deflate_lib
    return _deflate_lib


def test_header_symbols_exported(built):
    hdr = open(os.path.join(ROOT, "include", "rpcc_deflate.h")).read()
    declared = sorted(set(re.findall(r"\b(rpcc_[a-z0-9_]+)\s*\(", hdr)))
    assert declared == ["rpcc_deflate_bound", "rpcc_deflate_encode", "rpcc_deflate_last_error", "rpcc_deflate_version",
                        "rpcc_deflate_workspace_bytes"]
    lib = ctypes.CDLL(built.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    assert built.exported_symbols() == declared
    assert int(re.search(r"#define RPCC_DEFLATE_ABI_VERSION (\d+)", hdr).group(1)) == built.ABI_VERSION
    assert int(re.search(r"#define RPCC_DEFLATE_E_CAPACITY \(?(-?\d+)\)?", hdr).group(1)) == built.E_CAPACITY
    assert int(re.search(r"#define RPCC_DEFLATE_MAX_INPUT (0x[0-9A-F]+)", hdr).group(1), 16) == built.MAX_INPUT


def test_lz4_library_keeps_its_interface(built):
    from rpcc_amd import _lz4_lib
    assert _lz4_lib.lib().rpcc_lz4_version() == 1 and len(_lz4_lib.exported_symbols()) == 7


def test_version_bound_workspace(built):
    from rpcc_amd import deflate_codec
    lib = built.lib()
    assert lib.rpcc_deflate_version() == built.ABI_VERSION == 1
    for n in (0, 1, 65534, 65535, 65536, 131070, 131071, 188106, built.MAX_INPUT):
        assert lib.rpcc_deflate_bound(n) == 18 + n + 5 * max(1, -(-n // 65535)) == deflate_codec.bound(n)
    assert lib.rpcc_deflate_bound(-1) == 0
    assert lib.rpcc_deflate_bound(built.MAX_INPUT + 1) == 0
    assert lib.rpcc_deflate_workspace_bytes(1024, 1 << 20) >= 4 * ((1 << 20) + 1024)   # n + 1 records per stream
    assert lib.rpcc_deflate_workspace_bytes(3, 100) < lib.rpcc_deflate_workspace_bytes(4, 100) < lib.rpcc_deflate_workspace_bytes(4, 101)
    assert lib.rpcc_deflate_workspace_bytes(-1, 10) == 0
    assert lib.rpcc_deflate_workspace_bytes(1, -1) == 0


def test_argument_errors_do_not_crash(built):
    lib = built.lib()
    buf = ctypes.create_string_buffer(64)   # host memory: every call below must refuse before touching it
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.rpcc_deflate_encode(p, p, -1, 10, p, p, p, p, p, None) == -1
    assert b"bad argument" in lib.rpcc_deflate_last_error()
    assert lib.rpcc_deflate_encode(p, p, 4, -1, p, p, p, p, p, None) == -1
    assert b"bad argument" in lib.rpcc_deflate_last_error()
    for k in range(7):
        args = [p] * 7
        args[k] = None
        assert lib.rpcc_deflate_encode(args[0], args[1], 4, 100, args[2], args[3], args[4], args[5], args[6], None) == -1, k
        assert b"bad argument" in lib.rpcc_deflate_last_error()
    # nothing to do: no launch, no error
    assert lib.rpcc_deflate_encode(p, p, 0, 0, p, p, p, p, p, None) == 0


def test_source_digest_unchanged_by_the_deflate_library(built):
    from rpcc_amd import build as b
    before = b.source_digest()
    b.build_deflate(force=True)
    assert b.source_digest() == before
    for word in ("csrc_deflate", "csrc_lzmatch", "rpcc_deflate.h"):
        assert not any(word in d for d in b.DEPS), word
    assert os.path.exists(b.DEFLATE_LIB)
    # the match finder is a dependency of both entropy libraries and of nothing else
    shared = [d for d in b.LZ4_DEPS if "csrc_lzmatch" in d]
    assert shared and all(d in b.DEFLATE_DEPS for d in shared)
    assert not any("csrc_lzmatch" in d for d in b.EVAL_DEPS + b.SEG_DEPS)


def test_default_deflate_is_the_host_gzip():
    """Without device_entropy, 'deflate' and 'gzip' are gzip.compress, as before."""
    import rpcc_amd  # noqa: F401
    from rpcc_amd import compress_utils as cu
    a = np.arange(5000, dtype=np.int16) % 37
    for m in ("deflate", "gzip"):
        bc = cu.BasicCompressor(method_name=m)
        assert not bc.deflate_batched() and bc.batch_codec() is None
        want = gzip.compress(a)
        for got in (bc.compress(a), bc.compress_dict({"x": a})["x"]):
            assert got[:4] + got[8:] == want[:4] + want[8:]   # all but the header's time stamp
    assert cu.BasicCompressor(method_name="deflate", device_entropy=True).deflate_batched()
    assert not cu.BasicCompressor(method_name="bzip2", device_entropy=True).deflate_batched()
