"""csrc_inflate/inflate_core.h, the text the gfx950 decode kernel is compiled from, built for the host (tests/inflate_host_main.cpp) and
held to tests/inflate_ref.py: the same status, the same count and, where OK, the same bytes.
With a wave of one lane it runs every stream of tests/inflate_cases.py, plain and with -fsanitize=address,undefined.
With the kernel's own 64 lanes as threads (tests/host_wave.h) it runs inflate_cases.many_lane(), built plain, with
-fsanitize=address,undefined and with -fsanitize=thread: the barriers, ballots and shuffles as written, the bounds of the shared block
and the claims of INF_UNI.  What that cannot see is the code the compiler makes for gfx950, and speed.  The sanitizers' runtimes are
inside the programs.  No GPU needed."""
import os
import re
import struct
import subprocess

import pytest

import inflate_cases as C
import inflate_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZED = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
THREADS = ["-g", "-fsanitize=thread", "-static-libtsan"]
with open(os.path.join(ROOT, "r-pcc_amd", "csrc_inflate", "inflate_kernels.hip")) as _f:
    LANES = int(re.search(r"^#define INF_WAVE (\d+)$", _f.read(), re.M).group(1))


def _all_rows():
    rows = [(name, s, len(p)) for name, (s, p, _) in C.valid().items()]
    rows += [("flip%d" % k, s, cap) for k, (s, cap) in enumerate(C.flips())]
    rows += [("cut%d" % k, s, cap) for k, (s, cap) in enumerate(C.truncations())]
    rows += [(name, s, cap) for name, (s, cap, _) in C.hand_built().items()] + [("empty", b"", 0)]
    return rows


def _check(tmp_path, flags, rows):
    exe = str(tmp_path / "inflate_host")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-pthread"] + flags +
                          ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "r-pcc_amd", "csrc_inflate"),
                           os.path.join(ROOT, "tests", "inflate_host_main.cpp"), "-o", exe])
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<q", len(rows)))
        for _, s, cap in rows:
            f.write(struct.pack("<qq", len(s), cap) + s)
    run = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], stderr=subprocess.PIPE)
    assert run.returncode == 0 and not run.stderr, run.stderr.decode(errors="replace")[-4000:]      # a sanitizer's report, or host_wave's
    got = open(tmp_path / "out.bin", "rb").read()
    pos = 0
    for name, s, cap in rows:
        st, n = struct.unpack_from("<qq", got, pos)
        pos += 16
        want_st, want = R.inflate(s, cap=cap)
        assert (st, n) == (want_st, len(want)), (name, R.NAMES.get(st, st), R.NAMES[want_st])
        if st == R.OK:
            assert got[pos: pos + n] == want, name
            pos += n
    assert pos == len(got)


def test_host_build_of_the_kernel_text_equals_the_reference(tmp_path):
    _check(tmp_path, [], _all_rows())


def test_host_build_of_the_kernel_text_equals_the_reference_sanitized(tmp_path):
    _check(tmp_path, SANITIZED, _all_rows())


def test_the_many_lane_corpus_has_the_streams_that_cross_lanes():
    names = {name for name, _, _ in C.many_lane()}
    assert LANES == 64
    assert {"far_%d" % d for d in (32704, 32705, 32737, 32767, 32768)} <= names and {"near_%d" % d for d in (2, 3, 63, 64, 65)} <= names
    assert set(C.hand_built()) <= names


@pytest.mark.parametrize("flags", [[], SANITIZED, THREADS], ids=["plain", "address-undefined", "thread"])
def test_many_lane_host_build_equals_the_reference(tmp_path, flags):
    _check(tmp_path, flags + ["-DHOST_LANES=%d" % LANES], C.many_lane())
