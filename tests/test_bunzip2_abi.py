"""librpcc_bunzip2.so (include/rpcc_bunzip2.h) builds, exports what its header declares, reports its version, sizes the work slot by the
layout that carves it and refuses bad arguments before touching memory; csrc/, build.DEPS, source_digest() and the other libraries do
not change with it, and without device_bunzip2 nothing reaches it.  No GPU needed."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    import rpcc_amd  # noqa: F401
    from rpcc_amd import _bunzip2_lib
    return _bunzip2_lib


def test_header_symbols_exported(built):
    hdr = open(os.path.join(ROOT, "include", "rpcc_bunzip2.h")).read()
    declared = sorted(set(re.findall(r"\b(rpcc_bunzip2_[a-z0-9_]+)\s*\(", hdr.split("#ifndef RPCC_BUNZIP2_H")[1])))
    assert declared == ["rpcc_bunzip2_decode", "rpcc_bunzip2_last_error", "rpcc_bunzip2_stream_work_bytes", "rpcc_bunzip2_version"]
    lib = ctypes.CDLL(built.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    assert built.exported_symbols() == declared
    assert built.lib().rpcc_bunzip2_version() == built.ABI_VERSION == 1
    assert int(re.search(r"#define RPCC_BUNZIP2_ABI_VERSION (\d+)", hdr).group(1)) == built.ABI_VERSION
    macros = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define RPCC_BUNZIP2_(OK|E_[A-Z]+) \(?(-?\d+)\)?", hdr)}
    assert macros == {"OK": 0, "E_TRUNCATED": -2, "E_HEADER": -3, "E_MAGIC": -4, "E_RANDOMISED": -5, "E_TABLE": -6, "E_SYMBOL": -7,
                      "E_ORIGPTR": -8, "E_OVERRUN": -9, "E_CRC": -10, "E_WORK": -11, "E_TRAILING": -12, "E_RLE": -13}
    for name, value in macros.items():
        assert getattr(built, name) == value, name
    assert int(re.search(r"#define RPCC_BUNZIP2_MAX_BLOCK (\d+)", hdr).group(1)) == built.MAX_BLOCK == 900000


def test_reference_statuses_are_the_headers(built):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import bunzip2_ref as R
    from rpcc_amd import bunzip2_codec
    for value, name in R.NAMES.items():
        assert getattr(built, name) == value, name
        assert value == 0 or bunzip2_codec.status_text(value) != "error", name
    for level, cap in ((1, 0), (1, 10), (9, 188106), (9, 10 ** 7), (3, 239999), (3, 240000)):
        assert bunzip2_codec.block_bound(level, cap) == R.block_bound(level, cap)


def test_argument_errors_do_not_crash(built):
    lib = built.lib()
    buf = ctypes.create_string_buffer(64)   # host memory: every call below must refuse before touching it
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.rpcc_bunzip2_decode(p, p, -1, p, p, p, p, p, p, p, p, p, None) == -1
    assert b"bad argument" in lib.rpcc_bunzip2_last_error()
    assert lib.rpcc_bunzip2_decode(p, p, 0x80000000, p, p, p, p, p, p, p, p, p, None) == -1
    for k in range(11):
        args = [p] * 11
        args[k] = None
        assert lib.rpcc_bunzip2_decode(args[0], args[1], 4, *args[2:], None) == -1, k
        assert b"bad argument" in lib.rpcc_bunzip2_last_error()
    assert lib.rpcc_bunzip2_stream_work_bytes(-1) == -1
    # nothing to do: no launch, no error
    assert lib.rpcc_bunzip2_decode(p, p, 0, p, p, p, p, p, p, p, p, p, None) == 0


def test_stream_work_bytes_is_the_layouts(built, tmp_path):
    """Monotone, and what the layout function of bunzip2_core.h uses: the host build of the kernel text carves a heap block of exactly
    bz_work_layout(m).bytes, and tests/bunzip2_host_main.cpp refuses to run where bz_work_block does not invert it."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import bunzip2_ref as R
    lib = built.lib()
    sizes = [lib.rpcc_bunzip2_stream_work_bytes(m) for m in range(0, 2000)] + [lib.rpcc_bunzip2_stream_work_bytes(m) for m in (99999, 100000, 899999, 900000)]
    assert sizes[0] == 0 and all(a < b for a, b in zip(sizes, sizes[1:]))
    assert lib.rpcc_bunzip2_stream_work_bytes(900001) == lib.rpcc_bunzip2_stream_work_bytes(900000) == sizes[-1]
    for m in (0, 1, 63, 64, 1999, 100000, 900000):
        assert lib.rpcc_bunzip2_stream_work_bytes(m) == R.work_bytes(m)
    src, exe = tmp_path / "layout.cpp", str(tmp_path / "layout")
    # the wave of one lane as tests/bunzip2_host_main.cpp defines it, then a main that prints the layout and its inverse
    probe = ('#include <cstdio>\n#include <cstdint>\n#include <cstdlib>\n#include <cstring>\n#include "rpcc_bunzip2.h"\n' + open(os.path.join(ROOT, "tests", "bunzip2_host_main.cpp")).read()
             .split('#include "rpcc_bunzip2.h"')[1].split("int main")[0]
             + 'int main() { const int64_t m[] = {0, 1, 63, 64, 1999, 100000, 900000};\n'
               '  for (int64_t x : m) printf("%lld %lld %lld\\n", (long long)x, (long long)bz_work_layout(x).bytes, (long long)bz_work_block(bz_work_layout(x).bytes)); }\n')
    src.write_text(probe)
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O0", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "r-pcc_amd", "csrc_bunzip2"), str(src), "-o", exe])
    for line in subprocess.check_output([exe]).decode().split("\n")[:-1]:
        m, nbytes, back = map(int, line.split())
        assert lib.rpcc_bunzip2_stream_work_bytes(m) == nbytes and back == m, line


def test_source_digest_and_the_other_libraries_unchanged(built):
    from rpcc_amd import _deflate_lib, _inflate_lib, _lz4_lib, build as b
    before = b.source_digest()
    b.build_bunzip2(force=True)
    assert b.source_digest() == before
    assert os.path.exists(b.BUNZIP2_LIB)
    for deps in (b.DEPS, b.LZ4_DEPS, b.DEFLATE_DEPS, b.INFLATE_DEPS, b.EVAL_DEPS, b.SEG_DEPS):
        assert not any("csrc_bunzip2" in d or "rpcc_bunzip2.h" in d for d in deps)
    assert any("csrc_bunzip2" in d for d in b.BUNZIP2_DEPS)
    assert not any(x in d for d in b.BUNZIP2_DEPS for x in ("csrc_lzmatch", "csrc_deflate", "csrc_inflate", "csrc_lz4"))
    assert _lz4_lib.lib().rpcc_lz4_version() == 1 and len(_lz4_lib.exported_symbols()) == 7
    assert _deflate_lib.lib().rpcc_deflate_version() == 1 and len(_deflate_lib.exported_symbols()) == 5
    assert _inflate_lib.lib().rpcc_inflate_version() == 1 and len(_inflate_lib.exported_symbols()) == 3
    libs = set(os.listdir(os.path.dirname(b.BUNZIP2_LIB)))      # build() made the seven HIP libraries
    assert {"librpcc_bunzip2.so", "librpcc_deflate.so", "librpcc_eval.so", "librpcc_hip.so", "librpcc_inflate.so", "librpcc_lz4.so",
            "librpcc_seg.so"} <= libs


def test_without_device_bunzip2_the_decoder_is_not_imported():
    code = ("import sys, bz2, gzip, numpy as np\n"
            "import rpcc_amd\n"
            "from rpcc_amd import compress_utils as cu\n"
            "a = np.arange(5000, dtype=np.int16) % 37\n"
            "for m in cu.BasicCompressor.METHODS:\n"
            "    for ent in (False, True):\n"
            "        plain, flag = cu.BasicCompressor(method_name=m, device_entropy=ent), cu.BasicCompressor(method_name=m, device_entropy=ent, device_bunzip2=False)\n"
            "        assert (plain.batch_decoder() is None) == (flag.batch_decoder() is None) and not flag.device_bunzip2\n"
            "        if m != 'bzip2':\n"
            "            with_flag = cu.BasicCompressor(method_name=m, device_entropy=ent, device_bunzip2=True).batch_decoder()\n"
            "            assert with_flag is plain.batch_decoder() or with_flag == plain.batch_decoder()\n"
            "bc = cu.BasicCompressor(method_name='bzip2')\n"
            "assert bc.batch_decoder() is None and cu.BasicCompressor(method_name='bzip2', device_entropy=True).batch_decoder() is None\n"
            "assert bc.decompress(bz2.compress(a)) == a.tobytes()\n"
            "assert bc.decompress_dict({'x': bz2.compress(a)}) == {'x': a.tobytes()}\n"
            "assert bc.decompress_dicts([{'x': bz2.compress(a)}, {'y': bz2.compress(b'')}]) == [{'x': a.tobytes()}, {'y': b''}]\n"
            "assert not any(k.endswith('bunzip2_codec') or k.endswith('_bunzip2_lib') for k in sys.modules), sorted(sys.modules)\n"
            "on = cu.BasicCompressor(method_name='bzip2', device_bunzip2=True)\n"
            "assert on.batch_decoder().__module__.endswith('bunzip2_codec') and on.batch_decoder().__name__ == 'decompress_many'\n"
            "assert on.compress(a) == bz2.compress(a) and on.batch_codec() is None\n")
    subprocess.run([sys.executable, "-c", code], cwd=ROOT, check=True)


def test_tools_take_the_flag():
    code = ("import rpcc_amd\nfrom rpcc_amd.tools import compress as tc\n"
            "for dl in (False, True):\n"
            "    a = tc.make_parser(datalist=dl).parse_args(['--lidar', 'Velodyne64E', '--device_bunzip2'])\n"
            "    assert a.device_bunzip2 and tc.resolve_cfg(a)[4].device_bunzip2\n"
            "    a = tc.make_parser(datalist=dl).parse_args(['--lidar', 'Velodyne64E'])\n"
            "    assert not a.device_bunzip2 and not tc.resolve_cfg(a)[4].device_bunzip2\n")
    subprocess.run([sys.executable, "-c", code], cwd=ROOT, check=True)
