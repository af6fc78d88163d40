"""csrc_bzip2/bzip2_core.h, the text the gfx950 encode kernel is compiled from, built for the host with a workgroup of one thread
(tests/bzip2_host_main.cpp) and held to tests/bzip2_ref.py on every input of tests/bzip2_cases.py, those of several blocks at level 1
included: the same bytes.  What the 1024 threads do in parallel is the GPU tests' ground.  No GPU needed."""
import os
import struct
import subprocess

import bzip2_cases as C
import bzip2_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_build_of_the_kernel_text_equals_the_reference(tmp_path):
    exe = str(tmp_path / "bzip2_host")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "r-pcc_amd", "csrc_bzip2"), os.path.join(ROOT, "tests", "bzip2_host_main.cpp"), "-o", exe])
    cases = C.everything()
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<q", len(cases)))
        for x, level in cases.values():
            f.write(struct.pack("<qq", len(x), level) + x)
    subprocess.check_call([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
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
