"""csrc_bunzip2/bunzip2_core.h, the text the gfx950 decode kernel is compiled from, built for the host (tests/bunzip2_host_main.cpp) and
held to tests/bunzip2_ref.py: the same status, the same size, the same count of input bytes and, where OK or E_OVERRUN, the same bytes.
With a wave of one lane it runs every stream of tests/bunzip2_cases.py, plain and with -fsanitize=address,undefined.
With the kernel's own 64 lanes as threads (tests/host_wave.h) it runs bunzip2_cases.many_lane(), built plain, with
-fsanitize=address,undefined and with -fsanitize=thread: the barriers, ballots, shuffles and LDS atomics as written, the bounds of the
shared block and the work slot, and the claims of BZ_UNI.  What that cannot see is the code the compiler makes for gfx950, and speed.
The sanitizers' runtimes are inside the programs.  No GPU needed."""
import os
import re
import struct
import subprocess

import pytest

import bunzip2_cases as C
import bunzip2_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZED = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
THREADS = ["-g", "-fsanitize=thread", "-static-libtsan"]
with open(os.path.join(ROOT, "r-pcc_amd", "csrc_bunzip2", "bunzip2_kernels.hip")) as _f:
    LANES = int(re.search(r"^#define BZ_WAVE (\d+)$", _f.read(), re.M).group(1))


def rows():
    """-> [(name, stream, dst_cap, work block length)] over every case."""
    out = [(name, s, len(p), R.block_bound(int(s[3:4]), len(p))) for name, (s, p) in C.valid().items()]
    out += [("flip%d" % k, s, C.FLIP_CAP, C.FLIP_BLOCK) for k, s in enumerate(C.flips())]
    out += [("cut%d" % k, s, C.FLIP_CAP, C.FLIP_BLOCK) for k, s in enumerate(C.truncations())]
    out += [(name, s, cap, slot) for name, (s, cap, slot, _) in C.hand_built().items()] + [("empty", b"", 0, 0)]
    return out


def _check(tmp_path, flags, cases):
    exe = str(tmp_path / "bunzip2_host")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-pthread"] + flags +
                          ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "r-pcc_amd", "csrc_bunzip2"),
                           os.path.join(ROOT, "tests", "bunzip2_host_main.cpp"), "-o", exe])
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<q", len(cases)))
        for _, s, cap, slot in cases:
            f.write(struct.pack("<qqq", len(s), cap, slot) + s)
    run = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], stderr=subprocess.PIPE)
    assert run.returncode == 0 and not run.stderr, run.stderr.decode(errors="replace")[-4000:]      # a sanitizer's report, or host_wave's
    got = open(tmp_path / "out.bin", "rb").read()
    pos = 0
    for name, s, cap, slot in cases:
        st, n, used = struct.unpack_from("<qqq", got, pos)
        pos += 24
        want_st, want, size, want_used = R.bunzip2(s, cap=cap, nblock_max=slot)
        assert (st, n, used) == (want_st, size, want_used), (name, R.NAMES.get(st, st), R.NAMES[want_st])
        if st in (R.OK, R.E_OVERRUN):
            assert got[pos: pos + len(want)] == want, name
            pos += len(want)
    assert pos == len(got)


def test_host_build_of_the_kernel_text_equals_the_reference(tmp_path):
    _check(tmp_path, [], rows())


def test_host_build_of_the_kernel_text_equals_the_reference_sanitized(tmp_path):
    _check(tmp_path, SANITIZED, rows())


@pytest.mark.parametrize("flags", [[], SANITIZED, THREADS], ids=["plain", "address-undefined", "thread"])
def test_many_lane_host_build_equals_the_reference(tmp_path, flags):
    assert LANES == 64 and set(C.hand_built()) <= {name for name, _, _, _ in C.many_lane()}
    _check(tmp_path, flags + ["-DHOST_LANES=%d" % LANES], C.many_lane())
