"""librpcc_rans.so (include/rpcc_rans.h) builds, exports what its header declares, reports its version, bound and work buffer size, and
refuses bad arguments before touching memory; csrc/ and source_digest() do not change with it; basic_compressor 'rans' resolves to
rpcc_amd.rans_codec without loading the library, and the tools' parsers take the method.  No GPU needed."""
import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    import rpcc_amd  # noqa: F401
    from rpcc_amd import _rans_lib
    return _rans_lib


def test_header_symbols_exported(built):
    hdr = open(os.path.join(ROOT, "include", "rpcc_rans.h")).read()
    declared = sorted(set(re.findall(r"\b(rpcc_rans_[a-z0-9_]+)\s*\(", hdr)))
    assert declared == ["rpcc_rans_bound", "rpcc_rans_decode", "rpcc_rans_encode", "rpcc_rans_last_error", "rpcc_rans_version",
                        "rpcc_rans_workspace_bytes"]
    lib = ctypes.CDLL(built.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    assert built.exported_symbols() == declared
    assert int(re.search(r"#define RPCC_RANS_ABI_VERSION (\d+)", hdr).group(1)) == built.ABI_VERSION
    for name, val in (("OK", built.OK), ("E_CAPACITY", built.E_CAPACITY), ("E_HEADER", built.E_HEADER), ("E_TRUNCATED", built.E_TRUNCATED),
                      ("E_TABLE", built.E_TABLE), ("E_DIRECTORY", built.E_DIRECTORY), ("E_STATE", built.E_STATE), ("E_PAYLOAD", built.E_PAYLOAD)):
        assert int(re.search(r"#define RPCC_RANS_%s \(?(-?\d+)\)?" % name, hdr).group(1)) == val, name
    assert int(re.search(r"#define RPCC_RANS_MAX_INPUT (0x[0-9A-F]+)", hdr).group(1), 16) == built.MAX_INPUT
    assert int(re.search(r"#define RPCC_RANS_DEFAULT_CHUNK_LOG2 (\d+)", hdr).group(1)) == built.DEFAULT_CHUNK_LOG2
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import rans_ref as R
    assert (R.OK, R.E_CAPACITY, R.E_HEADER, R.E_TRUNCATED, R.E_TABLE, R.E_DIRECTORY, R.E_STATE, R.E_PAYLOAD, R.MAX_INPUT, R.DEFAULT_CHUNK_LOG2) == (
        built.OK, built.E_CAPACITY, built.E_HEADER, built.E_TRUNCATED, built.E_TABLE, built.E_DIRECTORY, built.E_STATE, built.E_PAYLOAD,
        built.MAX_INPUT, built.DEFAULT_CHUNK_LOG2)


def test_version_bound_workspace(built):
    lib = built.lib()
    assert lib.rpcc_rans_version() == built.ABI_VERSION == 1
    for n in (0, 1, 255, 65536, 188106, built.MAX_INPUT):
        assert lib.rpcc_rans_bound(n) == 12 + n
    assert lib.rpcc_rans_bound(-1) == 0
    assert lib.rpcc_rans_bound(built.MAX_INPUT + 1) == 0
    ws = lib.rpcc_rans_workspace_bytes
    # a scratch slot of 2 * chunk + 256 bytes for each of the 4 * (total / (4 * chunk) + nstreams) chunks the grid covers
    for n, total, clog in ((1, 0, 8), (4, 100000, 15), (1024, 135 << 20, 15), (3, 1 << 20, 16), (7, 12345, 8)):
        groups = total // (4 << clog) + n
        assert ws(n, total, clog) >= 4 * groups * (2 * (1 << clog) + 256) + n * (4096 + 2048 + 12)
        assert ws(n, total, clog) <= 4 * groups * (2 * (1 << clog) + 256 + 8) + n * (4096 + 2048 + 12) + 8 * 256
    assert ws(0, 0, 15) > 0
    for bad in ((-1, 0, 15), (1, -1, 15), (1, 0, 7), (1, 0, 17), (0x01000000, 0, 15)):
        assert ws(*bad) == 0, bad


def test_argument_errors_do_not_crash(built):
    lib = built.lib()
    buf = ctypes.create_string_buffer(64)   # host memory: every call below must refuse before touching it
    p = ctypes.cast(ctypes.addressof(buf) & ~15, ctypes.c_void_p)
    enc = lambda a, n=4, total=100, clog=15: lib.rpcc_rans_encode(a[0], a[1], p, n, total, clog, a[2], a[3], a[4], a[5], a[6], None)
    assert enc([p] * 7, n=-1) == -1
    assert b"bad argument" in lib.rpcc_rans_last_error()
    assert enc([p] * 7, total=-1) == -1 and enc([p] * 7, clog=7) == -1 and enc([p] * 7, clog=17) == -1
    for k in range(7):
        args = [p] * 7
        args[k] = None
        assert enc(args) == -1, k
    odd = ctypes.c_void_p(p.value + 8)
    assert enc([p] * 6 + [odd]) == -1                       # ws not at a multiple of 16
    assert lib.rpcc_rans_decode(p, p, -1, p, p, p, p, p, None) == -1
    for k in range(7):
        args = [p] * 7
        args[k] = None
        assert lib.rpcc_rans_decode(args[0], args[1], 4, args[2], args[3], args[4], args[5], args[6], None) == -1
    assert b"bad argument" in lib.rpcc_rans_last_error()
    # nothing to do: no launch, no error
    assert enc([p] * 7, n=0) == 0 and lib.rpcc_rans_decode(p, p, 0, p, p, p, p, p, None) == 0


def test_source_digest_unchanged_by_the_rans_library(built):
    from rpcc_amd import build as b
    before = b.source_digest()
    b.build_rans(force=True)
    assert b.source_digest() == before
    assert not any("csrc_rans" in d or d.endswith("rpcc_rans.h") or "librpcc_rans" in d for d in b.DEPS)
    assert os.path.exists(b.RANS_LIB)
    assert any(d.endswith("rans_core.h") for d in b.RANS_DEPS) and any(d.endswith("rpcc_rans.h") for d in b.RANS_DEPS)


def test_basic_compressor_names_the_codec_without_loading_the_library():
    import rpcc_amd  # noqa: F401
    from rpcc_amd import _rans_lib, compress_utils as cu, rans_codec
    loaded = _rans_lib._b._h
    assert "rans" in cu.BasicCompressor.METHODS and cu.BACKENDS["rans"].host_encode is None
    for flags in ({}, dict(device_entropy=True, device_bunzip2=True, device_bzip2=True)):
        bc = cu.BasicCompressor(method_name="rans", **flags)
        assert bc.batch_codec() == (rans_codec, rans_codec.compress_many) and bc.batch_decoder() is rans_codec.decompress_many
        assert not (bc.lz4_batched() or bc.deflate_batched() or bc.bzip2_batched())
    bc = cu.BasicCompressor()
    bc.set_method("rans")
    assert bc.method_name == "rans"
    assert _rans_lib._b._h is loaded                        # nothing above reached the library
    assert cu.BasicCompressor(method_name="bzip2").batch_codec() is None     # the default's resolution is what it was
    with pytest.raises(AssertionError, match="lz4, bzip2, gzip, deflate, rans"):
        cu.BasicCompressor(method_name="zstd")
    assert rans_codec.bound(0) == 12 and rans_codec.bound(1000) == 1012


@pytest.mark.parametrize("tool", ["compress", "compress_datalist", "decompress", "decompress_datalist"])
def test_tool_parsers_accept_the_method(tool):
    import importlib
    import rpcc_amd  # noqa: F401
    mod = importlib.import_module("rpcc_amd.tools." + tool)
    args = mod.make_parser(datalist=tool.endswith("datalist")).parse_args(["--basic_compressor", "rans"])
    assert args.basic_compressor == "rans"
    bc = importlib.import_module("rpcc_amd.tools.compress").resolve_cfg(args)[4]      # what every tool makes of its arguments
    assert bc.method_name == "rans" and bc.batch_codec()[0].__name__.endswith(".rans_codec")
