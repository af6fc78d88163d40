"""librpcc_inflate.so (include/rpcc_inflate.h) builds, exports what its header declares, reports its version and refuses bad
arguments before touching memory; csrc/, build.DEPS, source_digest() and the other entropy libraries do not change with it, and
without device_entropy nothing reaches it.  No GPU needed."""
import ctypes
import gzip
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    import rpcc_amd  # noqa: F401
    from rpcc_amd import _inflate_lib
    return _inflate_lib


def test_header_symbols_exported(built):
    hdr = open(os.path.join(ROOT, "include", "rpcc_inflate.h")).read()
    declared = sorted(set(re.findall(r"\b(rpcc_[a-z0-9_]+)\s*\(", hdr)))
    assert declared == ["rpcc_inflate_decode", "rpcc_inflate_last_error", "rpcc_inflate_version"]
    lib = ctypes.CDLL(built.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    assert built.exported_symbols() == declared
    assert built.lib().rpcc_inflate_version() == built.ABI_VERSION == 1
    assert int(re.search(r"#define RPCC_INFLATE_ABI_VERSION (\d+)", hdr).group(1)) == built.ABI_VERSION
    macros = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define RPCC_INFLATE_(OK|E_[A-Z]+) \(?(-?\d+)\)?", hdr)}
    assert macros == {"OK": 0, "E_TRUNCATED": -2, "E_HEADER": -3, "E_BTYPE": -4, "E_STORED": -5, "E_TABLE": -6, "E_SYMBOL": -7,
                      "E_OFFSET": -8, "E_OVERRUN": -9, "E_CRC": -10, "E_SIZE": -11, "E_TRAILING": -12}
    for name, value in macros.items():
        assert getattr(built, name) == value, name
    assert int(re.search(r"#define RPCC_INFLATE_MAX_STREAMS (0x[0-9A-F]+)", hdr).group(1), 16) == 0x7FFFFFFF


def test_reference_statuses_are_the_headers(built):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import inflate_ref as R
    from rpcc_amd import inflate_codec
    for value, name in R.NAMES.items():
        assert getattr(built, name) == value, name
        assert value == 0 or inflate_codec.status_text(value) != "error", name


def test_argument_errors_do_not_crash(built):
    lib = built.lib()
    buf = ctypes.create_string_buffer(64)   # host memory: every call below must refuse before touching it
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.rpcc_inflate_decode(p, p, -1, p, p, p, p, p, None) == -1
    assert b"bad argument" in lib.rpcc_inflate_last_error()
    assert lib.rpcc_inflate_decode(p, p, 0x80000000, p, p, p, p, p, None) == -1
    for k in range(7):
        args = [p] * 7
        args[k] = None
        assert lib.rpcc_inflate_decode(args[0], args[1], 4, args[2], args[3], args[4], args[5], args[6], None) == -1, k
        assert b"bad argument" in lib.rpcc_inflate_last_error()
    # nothing to do: no launch, no error
    assert lib.rpcc_inflate_decode(p, p, 0, p, p, p, p, p, None) == 0


def test_source_digest_and_the_other_libraries_unchanged(built):
    from rpcc_amd import _deflate_lib, _lz4_lib, build as b
    before = b.source_digest()
    b.build_inflate(force=True)
    assert b.source_digest() == before
    assert os.path.exists(b.INFLATE_LIB)
    for deps in (b.DEPS, b.LZ4_DEPS, b.DEFLATE_DEPS, b.EVAL_DEPS, b.SEG_DEPS):
        assert not any("csrc_inflate" in d or "rpcc_inflate.h" in d for d in deps)
    assert any("csrc_inflate" in d for d in b.INFLATE_DEPS) and not any("csrc_lzmatch" in d or "csrc_deflate" in d for d in b.INFLATE_DEPS)
    assert _lz4_lib.lib().rpcc_lz4_version() == 1 and len(_lz4_lib.exported_symbols()) == 7
    assert _deflate_lib.lib().rpcc_deflate_version() == 1 and len(_deflate_lib.exported_symbols()) == 5


def test_size_fields():
    """The slot sizes decode_many takes from a member's last bytes: the stated size when nothing follows, an upper bound of it when zero bytes do."""
    import rpcc_amd  # noqa: F401
    from rpcc_amd import inflate_codec as ic
    for n in (0, 1, 255, 256, 65536, 188106, 1 << 24):
        m = np.frombuffer(gzip.compress(bytes(n), 1), np.uint8)
        assert ic.size_fields(m)[0] == n
        for pad in (1, 2, 3, 4, 9):
            alone, padded = ic.size_fields(np.concatenate([m, np.zeros(pad, np.uint8)]))
            assert alone <= n <= padded <= ic.MAX_RATIO * (m.size + pad), (n, pad)
    m = np.frombuffer(gzip.compress(b"abc")[:-4] + b"\xff\xff\xff\x7f", np.uint8)      # a lying size is capped at deflate's largest ratio
    assert ic.size_fields(m) == (ic.MAX_RATIO * m.size,) * 2
    assert ic.size_fields(m[:17]) == (0, 0)


def test_without_device_entropy_the_decoder_is_not_imported():
    code = ("import sys, gzip, numpy as np\n"
            "import rpcc_amd\n"
            "from rpcc_amd import compress_utils as cu\n"
            "a = np.arange(5000, dtype=np.int16) % 37\n"
            "for m in ('deflate', 'gzip'):\n"
            "    bc = cu.BasicCompressor(method_name=m)\n"
            "    assert bc.batch_decoder() is None\n"
            "    assert bc.decompress(gzip.compress(a)) == a.tobytes()\n"
            "    assert bc.decompress_dict({'x': gzip.compress(a)}) == {'x': a.tobytes()}\n"
            "    assert bc.decompress_dicts([{'x': gzip.compress(a)}, {'y': gzip.compress(b'')}]) == [{'x': a.tobytes()}, {'y': b''}]\n"
            "assert cu.BasicCompressor(method_name='bzip2', device_entropy=True).batch_decoder() is None\n"
            "assert not any(k.endswith('inflate_codec') or k.endswith('_inflate_lib') for k in sys.modules), sorted(sys.modules)\n"
            "assert cu.BasicCompressor(method_name='deflate', device_entropy=True).batch_decoder().__module__.endswith('inflate_codec')\n")
    subprocess.run([sys.executable, "-c", code], cwd=ROOT, check=True)
