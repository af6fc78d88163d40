"""librpcc_bzip2.so (include/rpcc_bzip2.h) builds, exports what its header declares, reports its version, states its bound and its work
layout as tests/bzip2_ref.py and rpcc_amd.bzip2_codec do, and refuses bad arguments before touching memory; csrc/, build.DEPS,
source_digest() and the other libraries do not change with it, and without device_bzip2 nothing reaches it.  No GPU needed."""
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
    from rpcc_amd import _bzip2_lib
    return _bzip2_lib


def test_header_symbols_exported(built):
    hdr = open(os.path.join(ROOT, "include", "rpcc_bzip2.h")).read()
    declared = sorted(set(re.findall(r"\b(rpcc_bzip2_[a-z0-9_]+)\s*\(", hdr.split("#ifndef RPCC_BZIP2_H")[1])))
    assert declared == ["rpcc_bzip2_bound", "rpcc_bzip2_encode", "rpcc_bzip2_last_error", "rpcc_bzip2_version", "rpcc_bzip2_workspace_bytes"]
    lib = ctypes.CDLL(built.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    assert built.exported_symbols() == declared
    assert built.lib().rpcc_bzip2_version() == built.ABI_VERSION == 1
    assert int(re.search(r"#define RPCC_BZIP2_ABI_VERSION (\d+)", hdr).group(1)) == built.ABI_VERSION
    assert int(re.search(r"#define RPCC_BZIP2_E_CAPACITY \((-?\d+)\)", hdr).group(1)) == built.E_CAPACITY == -1
    assert int(re.search(r"#define RPCC_BZIP2_MAX_INPUT (0x[0-9A-Fa-f]+)", hdr).group(1), 16) == built.MAX_INPUT
    assert (int(re.search(r"#define RPCC_BZIP2_ERR_ARG \((-?\d+)\)", hdr).group(1)), int(re.search(r"#define RPCC_BZIP2_ERR_HIP \((-?\d+)\)", hdr).group(1))) == (-1, -2)


def test_argument_errors_do_not_crash(built):
    lib = built.lib()
    buf = ctypes.create_string_buffer(64)   # host memory: every call below must refuse before touching it
    p = ctypes.cast(buf, ctypes.c_void_p)
    a16 = ctypes.c_void_p((p.value + 15) & ~15)
    assert lib.rpcc_bzip2_encode(p, p, -1, 0, 9, p, p, p, p, a16, None) == -1
    assert b"bad argument" in lib.rpcc_bzip2_last_error()
    assert lib.rpcc_bzip2_encode(p, p, 0x80000000, 0, 9, p, p, p, p, a16, None) == -1
    assert lib.rpcc_bzip2_encode(p, p, 4, -1, 9, p, p, p, p, a16, None) == -1
    assert lib.rpcc_bzip2_encode(p, p, 4, (1 << 36) + 1, 9, p, p, p, p, a16, None) == -1
    for level in (0, 10, -1):
        assert lib.rpcc_bzip2_encode(p, p, 4, 100, level, p, p, p, p, a16, None) == -1
    for k in range(7):
        args = [p, p, p, p, p, p, a16]
        args[k] = None
        assert lib.rpcc_bzip2_encode(args[0], args[1], 4, 100, 9, *args[2:], None) == -1, k
        assert b"bad argument" in lib.rpcc_bzip2_last_error()
    assert lib.rpcc_bzip2_encode(p, p, 4, 100, 9, p, p, p, p, ctypes.c_void_p(a16.value + 8), None) == -1   # ws not 16-byte aligned
    # nothing to do: no launch, no error
    assert lib.rpcc_bzip2_encode(p, p, 0, 0, 9, p, p, p, p, a16, None) == 0
    assert lib.rpcc_bzip2_workspace_bytes(-1, 0, 9) == 0 and lib.rpcc_bzip2_workspace_bytes(1, -1, 9) == 0
    assert lib.rpcc_bzip2_workspace_bytes(1, 1, 0) == 0 and lib.rpcc_bzip2_workspace_bytes(1, 1, 10) == 0
    assert lib.rpcc_bzip2_bound(-1, 9) == 0 and lib.rpcc_bzip2_bound(built.MAX_INPUT + 1, 9) == 0 and lib.rpcc_bzip2_bound(5, 0) == 0


def test_bound_and_work_layout_agree(built, tmp_path):
    """rpcc_bzip2_bound, rpcc_bzip2_workspace_bytes and the layout of bzip2_core.h against their statements in tests/bzip2_ref.py and
    rpcc_amd/bzip2_codec.py; the call's bound of the slots covers every slot."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import bzip2_ref as R
    from rpcc_amd import bzip2_codec
    lib = built.lib()
    sizes = (0, 1, 3, 4, 50, 1000, 79984, 79985, 79986, 99981, 188106, 719984, 719985, 900000, 10 ** 7, built.MAX_INPUT)
    for level in (1, 5, 9):
        for n in sizes:
            assert lib.rpcc_bzip2_bound(n, level) == R.bound(n, level) == bzip2_codec.bound(n, level) > n, (n, level)
        for ns, total in ((1, 0), (1, 1), (4, 217872), (1024, 55775232), (3, 10 ** 9)):
            assert lib.rpcc_bzip2_workspace_bytes(ns, total, level) == R.workspace_bytes(ns, total) == bzip2_codec.workspace_bytes(ns, total, level)
    assert R.bound(0) == 14 + 6450 + 3 and bzip2_codec.block_limit(1) == R.block_limit(1) == 99981
    src, exe = tmp_path / "layout.cpp", str(tmp_path / "layout")
    # the workgroup of one thread as tests/bzip2_host_main.cpp defines it, then a main that prints the layout
    probe = ('#include <cstdio>\n#include <cstdint>\n#include <cstdlib>\n#include <cstring>\n#include "rpcc_bzip2.h"\n' + open(os.path.join(ROOT, "tests", "bzip2_host_main.cpp")).read()
             .split('#include "rpcc_bzip2.h"')[1].split("int main")[0]
             + 'int main() { const int64_t m[] = {0, 1, 15, 16, 17, 255, 256, 257, 1999, 99981, 235132, 899981};\n'
               '  for (int64_t x : m) { const BzeLayout w = bze_layout(x);\n'
               '    printf("%lld %lld %lld %lld\\n", (long long)x, (long long)w.bytes, (long long)(w.states + 256 * ((x + 255) / 256)), (long long)w.sa2); } }\n')
    src.write_text(probe)
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O0", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "r-pcc_amd", "csrc_bzip2"), str(src), "-o", exe])
    for line in subprocess.check_output([exe]).decode().split("\n")[:-1]:
        m, nbytes, chunks_end, sa2 = map(int, line.split())
        assert nbytes == R.work_bytes(m) and chunks_end <= nbytes and sa2 >= 4 * m and nbytes % 16 == 0, line
        assert nbytes <= 23 * max(16, (m + 15) // 16 * 16) + 576, line
    # the slots of any set of streams fit the call's bound of them
    for lens in ([0], [1], [3] * 7, [188106, 12134, 16000, 1632], [10 ** 6, 5], [79985] * 3):
        for level in (1, 9):
            slots = sum(R.work_bytes(R.block_cap(n, level)) for n in lens)
            assert (8 * len(lens) + 255) // 256 * 256 + slots <= R.workspace_bytes(len(lens), sum(lens)), (lens, level)


def test_source_digest_and_the_other_libraries_unchanged(built):
    from rpcc_amd import _bunzip2_lib, _deflate_lib, build as b
    before = b.source_digest()
    b.build_bzip2(force=True)
    assert b.source_digest() == before
    assert os.path.exists(b.BZIP2_LIB)
    for deps in (b.DEPS, b.LZ4_DEPS, b.DEFLATE_DEPS, b.INFLATE_DEPS, b.BUNZIP2_DEPS, b.EVAL_DEPS, b.SEG_DEPS):
        assert not any("csrc_bzip2" in d or "rpcc_bzip2.h" in d for d in deps)
    assert any("csrc_bzip2" in d for d in b.BZIP2_DEPS)
    assert not any(x in d for d in b.BZIP2_DEPS for x in ("csrc_lzmatch", "csrc_deflate", "csrc_inflate", "csrc_lz4", "csrc_bunzip2"))
    assert sorted(os.path.basename(d) for d in b.DEPS if d.endswith(("rpcc_hip.hip", "rpcc_hip.h"))) == ["rpcc_hip.h", "rpcc_hip.hip"]
    assert all(os.path.dirname(d) in (os.path.join(ROOT, "r-pcc_amd", "csrc"), os.path.join(ROOT, "include")) for d in b.DEPS)
    assert _deflate_lib.lib().rpcc_deflate_version() == 1 and len(_deflate_lib.exported_symbols()) == 5
    assert _bunzip2_lib.lib().rpcc_bunzip2_version() == 1 and len(_bunzip2_lib.exported_symbols()) == 4


def test_without_device_bzip2_the_encoder_is_not_imported():
    code = ("import sys, bz2, numpy as np\n"
            "import rpcc_amd\n"
            "from rpcc_amd import compress_utils as cu, pipeline\n"
            "a = np.arange(5000, dtype=np.int16) % 37\n"
            "for m in cu.BasicCompressor.METHODS:\n"
            "    for ent in (False, True):\n"
            "        plain, flag = cu.BasicCompressor(method_name=m, device_entropy=ent), cu.BasicCompressor(method_name=m, device_entropy=ent, device_bzip2=False)\n"
            "        assert not flag.device_bzip2 and not flag.bzip2_batched()\n"
            "        if m != 'bzip2':\n"
            "            on = cu.BasicCompressor(method_name=m, device_entropy=ent, device_bzip2=True)\n"
            "            assert not on.bzip2_batched() and (on.batch_codec() is None) == (plain.batch_codec() is None)\n"
            "bc = cu.BasicCompressor(method_name='bzip2')\n"
            "assert bc.batch_codec() is None and cu.BasicCompressor(method_name='bzip2', device_entropy=True, device_bunzip2=True).batch_codec() is None\n"
            "assert bc.compress(a) == bz2.compress(a) and bc.compress_dict({'x': a}) == {'x': bz2.compress(a)}\n"
            "od = {'contour_map': a.view(np.uint8), 'idx_sequence': a.view(np.uint16), 'plane_param': np.ones(8, np.float32), 'residual_quantized': a}\n"
            "assert cu.pack_frames(bc, [od]) == [cu.pack_bitstream({k: bz2.compress(v) for k, v in od.items()})]\n"
            "assert not any(k.endswith('bzip2_codec') and not k.endswith('bunzip2_codec') or k.endswith('._bzip2_lib') for k in sys.modules), sorted(sys.modules)\n"
            "on = cu.BasicCompressor(method_name='bzip2', device_bzip2=True)\n"
            "assert on.bzip2_batched() and on.batch_codec()[0].__name__.endswith('.bzip2_codec') and on.batch_codec()[1].__name__ == 'compress_many'\n"
            "assert on.batch_decoder() is None and on.decompress(bz2.compress(a)) == a.tobytes()\n")
    subprocess.run([sys.executable, "-c", code], cwd=ROOT, check=True)


def test_tools_take_the_flag():
    code = ("import rpcc_amd\nfrom rpcc_amd.tools import compress as tc\n"
            "for dl in (False, True):\n"
            "    a = tc.make_parser(datalist=dl).parse_args(['--lidar', 'Velodyne64E', '--device_bzip2'])\n"
            "    assert a.device_bzip2 and tc.resolve_cfg(a)[4].device_bzip2 and tc.resolve_cfg(a)[4].bzip2_batched()\n"
            "    a = tc.make_parser(datalist=dl).parse_args(['--lidar', 'Velodyne64E'])\n"
            "    assert not a.device_bzip2 and not tc.resolve_cfg(a)[4].device_bzip2\n")
    subprocess.run([sys.executable, "-c", code], cwd=ROOT, check=True)
