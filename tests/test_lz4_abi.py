"""librpcc_lz4.so (include/rpcc_lz4.h) builds, exports what its header declares, reports its version and bound, and refuses bad
arguments before touching memory; csrc/ and source_digest() do not change with it.  No GPU needed."""
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
    from rpcc_amd import _lz4_lib
    return _lz4_lib


def test_header_symbols_exported(built):
    hdr = open(os.path.join(ROOT, "include", "rpcc_lz4.h")).read()
    declared = sorted(set(re.findall(r"\b(rpcc_[a-z0-9_]+)\s*\(", hdr)))
    assert len(declared) == 7
    lib = ctypes.CDLL(built.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    assert built.exported_symbols() == declared
    assert int(re.search(r"#define RPCC_LZ4_ABI_VERSION (\d+)", hdr).group(1)) == built.ABI_VERSION
    for name, val in (("RPCC_LZ4_OK", built.OK), ("RPCC_LZ4_E_CAPACITY", built.E_CAPACITY), ("RPCC_LZ4_E_TRUNCATED", built.E_TRUNCATED),
                      ("RPCC_LZ4_E_OFFSET", built.E_OFFSET), ("RPCC_LZ4_E_OVERRUN", built.E_OVERRUN), ("RPCC_LZ4_E_SIZE", built.E_SIZE)):
        assert int(re.search(r"#define %s \(?(-?\d+)\)?" % name, hdr).group(1)) == val, name
    assert int(re.search(r"#define RPCC_LZ4_MAX_INPUT (0x[0-9A-F]+)", hdr).group(1), 16) == built.MAX_INPUT


def test_version_bound_workspace(built):
    lib = built.lib()
    assert lib.rpcc_lz4_version() == built.ABI_VERSION == 1
    for n in (0, 1, 254, 255, 65536, 188106, built.MAX_INPUT):
        assert lib.rpcc_lz4_bound(n) == 4 + n + n // 255 + 16
    assert lib.rpcc_lz4_bound(-1) == 0
    assert lib.rpcc_lz4_bound(built.MAX_INPUT + 1) == 0
    assert lib.rpcc_lz4_workspace_bytes(1280) >= 1281 * 8
    assert lib.rpcc_lz4_workspace_bytes(-1) == 0


def test_argument_errors_do_not_crash(built):
    lib = built.lib()
    buf = ctypes.create_string_buffer(64)   # host memory: every call below must refuse before touching it
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.rpcc_lz4_encode(p, p, -1, p, p, p, p, None) == -1
    assert b"bad argument" in lib.rpcc_lz4_last_error()
    for k in range(6):
        args = [p] * 6
        args[k] = None
        assert lib.rpcc_lz4_encode(args[0], args[1], 4, args[2], args[3], args[4], args[5], None) == -1
    assert lib.rpcc_lz4_decode(p, p, -1, p, p, p, p, p, None) == -1
    for k in range(7):
        args = [p] * 7
        args[k] = None
        assert lib.rpcc_lz4_decode(args[0], args[1], 4, args[2], args[3], args[4], args[5], args[6], None) == -1
    assert lib.rpcc_lz4_pack_containers(p, p, p, -1, 4, p, 100, p, p, p, None) == -1
    assert lib.rpcc_lz4_pack_containers(p, p, p, 2, 0, p, 100, p, p, p, None) == -1
    assert lib.rpcc_lz4_pack_containers(p, p, p, 2, 4, p, -1, p, p, p, None) == -1
    assert lib.rpcc_lz4_pack_containers(p, p, p, 2, 4, p, 100, p, p, None, None) == -1
    assert b"bad argument" in lib.rpcc_lz4_last_error()
    # nothing to do: no launch, no error
    assert lib.rpcc_lz4_encode(p, p, 0, p, p, p, p, None) == 0


def test_source_digest_unchanged_by_the_lz4_library(built):
    from rpcc_amd import build as b
    before = b.source_digest()
    b.build_lz4(force=True)
    assert b.source_digest() == before
    assert not any("csrc_lz4" in d or d.endswith("rpcc_lz4.h") for d in b.DEPS)
    assert os.path.exists(b.LZ4_LIB)


def test_basic_compressor_falls_back_to_the_codec():
    """Without the lz4 package, basic_compressor 'lz4' resolves to rpcc_amd.lz4_codec instead of raising."""
    import rpcc_amd  # noqa: F401
    from rpcc_amd import compress_utils as cu
    try:
        import lz4  # noqa: F401
        pytest.skip("the lz4 package is installed: it is used, as before")
    except ImportError:
        pass
    from rpcc_amd import lz4_codec
    bc = cu.BasicCompressor(method_name="lz4")
    assert bc._lz4() is lz4_codec and bc.lz4_batched()
    assert not cu.BasicCompressor(method_name="bzip2").lz4_batched()
