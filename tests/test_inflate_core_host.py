"""csrc_inflate/inflate_core.h, the text the gfx950 decode kernel is compiled from, built for the host with a wave of one lane
(tests/inflate_host_main.cpp) and held to tests/inflate_ref.py on every stream of tests/inflate_cases.py: the same status, the same
count and, where OK, the same bytes.  What the 64 lanes do in parallel is the GPU tests' ground.  No GPU needed."""
import os
import struct
import subprocess

import inflate_cases as C
import inflate_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_build_of_the_kernel_text_equals_the_reference(tmp_path):
    exe = str(tmp_path / "inflate_host")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "r-pcc_amd", "csrc_inflate"), os.path.join(ROOT, "tests", "inflate_host_main.cpp"), "-o", exe])
    rows = [(name, s, len(p)) for name, (s, p, _) in C.valid().items()]
    rows += [("flip%d" % k, s, cap) for k, (s, cap) in enumerate(C.flips())]
    rows += [("cut%d" % k, s, cap) for k, (s, cap) in enumerate(C.truncations())]
    rows += [(name, s, cap) for name, (s, cap, _) in C.hand_built().items()] + [("empty", b"", 0)]
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<q", len(rows)))
        for _, s, cap in rows:
            f.write(struct.pack("<qq", len(s), cap) + s)
    subprocess.check_call([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
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
