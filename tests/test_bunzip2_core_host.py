"""csrc_bunzip2/bunzip2_core.h, the text the gfx950 decode kernel is compiled from, built for the host with a wave of one lane
(tests/bunzip2_host_main.cpp) and held to tests/bunzip2_ref.py on every stream of tests/bunzip2_cases.py: the same status, the same
size, the same count of input bytes and, where OK or E_OVERRUN, the same bytes.  What the 64 lanes do in parallel is the GPU tests'
ground.  No GPU needed."""
import os
import struct
import subprocess

import bunzip2_cases as C
import bunzip2_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rows():
    """-> [(name, stream, dst_cap, work block length)] over every case."""
    out = [(name, s, len(p), R.block_bound(int(s[3:4]), len(p))) for name, (s, p) in C.valid().items()]
    out += [("flip%d" % k, s, C.FLIP_CAP, C.FLIP_BLOCK) for k, s in enumerate(C.flips())]
    out += [("cut%d" % k, s, C.FLIP_CAP, C.FLIP_BLOCK) for k, s in enumerate(C.truncations())]
    out += [(name, s, cap, slot) for name, (s, cap, slot, _) in C.hand_built().items()] + [("empty", b"", 0, 0)]
    return out


def test_host_build_of_the_kernel_text_equals_the_reference(tmp_path):
    exe = str(tmp_path / "bunzip2_host")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "r-pcc_amd", "csrc_bunzip2"), os.path.join(ROOT, "tests", "bunzip2_host_main.cpp"), "-o", exe])
    cases = rows()
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<q", len(cases)))
        for _, s, cap, slot in cases:
            f.write(struct.pack("<qqq", len(s), cap, slot) + s)
    subprocess.check_call([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
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
