"""csrc_bzip2/bzip2_core.h, the text the gfx950 encode kernel is compiled from, built for the host (tests/bzip2_host_main.cpp) and held
to tests/bzip2_ref.py: the same bytes, the same bound and work-slot size.
With a workgroup of one thread it runs every input of tests/bzip2_cases.py, those of several blocks at level 1 included, plain and
with -fsanitize=address,undefined.
With the kernel's own 1024 threads in waves of 64 (tests/host_wave.h) it runs bzip2_cases.many_thread(), built plain, with
-fsanitize=address,undefined and with -fsanitize=thread: the barriers, ballots, shuffles and LDS atomics as written, and the bounds of
the shared block and the work slot.  What that cannot see is the code the compiler makes for gfx950, and speed.  The sanitizers'
runtimes are inside the programs.  No GPU needed."""
import os
import re
import struct
import subprocess

import pytest

import bunzip2_ref
import bzip2_cases as C
import bzip2_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZED = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
THREADS = ["-g", "-fsanitize=thread", "-static-libtsan"]
with open(os.path.join(ROOT, "r-pcc_amd", "csrc_bzip2", "bzip2_kernels.hip")) as _f:
    _hip = _f.read()
BZE_T = int(re.search(r"^#define BZE_T (\d+)$", _hip, re.M).group(1))
BZE_WAVE = int(re.search(r"^#define BZE_WAVE (\d+)$", _hip, re.M).group(1))


def _check(tmp_path, flags, cases):
    exe = str(tmp_path / "bzip2_host")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-pthread"] + flags +
                          ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "r-pcc_amd", "csrc_bzip2"),
                           os.path.join(ROOT, "tests", "bzip2_host_main.cpp"), "-o", exe])
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<q", len(cases)))
        for x, level in cases.values():
            f.write(struct.pack("<qq", len(x), level) + x)
    run = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], stderr=subprocess.PIPE)
    assert run.returncode == 0 and not run.stderr, run.stderr.decode(errors="replace")[-4000:]      # a sanitizer's report, or host_wave's
    got = open(tmp_path / "out.bin", "rb").read()
    pos = 0
    for name, (x, level) in cases.items():
        n, cap, work = struct.unpack_from("<qqq", got, pos)
        pos += 24
        assert cap == R.bound(len(x), level) and work == R.work_bytes(R.block_cap(len(x), level)), name
        want = R.compress(x, level)
        assert n == len(want) and got[pos: pos + n] == want, name
        pos += n
    assert pos == len(got)


def test_host_build_of_the_kernel_text_equals_the_reference(tmp_path):
    _check(tmp_path, [], C.everything())


def test_host_build_of_the_kernel_text_equals_the_reference_sanitized(tmp_path):
    _check(tmp_path, SANITIZED, C.everything())


def test_the_many_thread_inputs_are_what_they_are_there_for():
    x, level = C.many_thread()["two_blocks"]
    assert (BZE_T, BZE_WAVE) == (1024, 64) and level == 1
    assert bunzip2_ref.bunzip2(R.compress(x, level), report=True)[4]["blocks"] == 2 and R.block_cap(len(x), level) == 99981


@pytest.mark.parametrize("flags", [[], SANITIZED, THREADS], ids=["plain", "address-undefined", "thread"])
def test_many_thread_host_build_equals_the_reference(tmp_path, flags):
    _check(tmp_path, flags + ["-DHOST_T=%d" % BZE_T, "-DHOST_WAVE=%d" % BZE_WAVE], C.many_thread())
