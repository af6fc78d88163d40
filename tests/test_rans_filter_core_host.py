"""csrc_rans/rans_core.h with csrc_rans/rans_filter.h, the text the gfx950 kernels are compiled from, built for the host with the wave
emulated lane by lane (tests/rans_filter_host_main.cpp) and held to tests/rans_filter_ref.py over tests/rans_filter_cases.py: every case
encodes to the reference's bytes (with the stored fallback and without it), every valid, forced and hostile stream decodes to the
reference's status, count and bytes.  The same program is built once more with -fsanitize=address,undefined (runtimes inside the
program) and run over the same table.  No GPU needed."""
import os
import struct
import subprocess

import pytest

import rans_filter_cases as C
import rans_filter_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rows():
    """-> [(name, op, header ints, bytes)]"""
    rows = []
    for name, (d, w, c, f) in C.valid().items():
        rows.append((name, 0, (len(d), w, c, 1, f), d))
        if name in C.forced():
            rows.append((name, 0, (len(d), w, c, 0, f), d))
    for name, (d, w, c, f) in C.valid().items():
        s = C.reference(name)
        rows.append((name, 1, (len(s), len(d)), s))
    for name, (s, d) in C.forced().items():
        rows.append((name, 1, (len(s), len(d)), s))
    for name, (s, cap) in C.hostile().items():
        rows.append((name, 1, (len(s), cap), s))
    return rows


@pytest.mark.parametrize("flags", [["-O1"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                                      "-static-libasan", "-static-libubsan"]], ids=["plain", "sanitized"])
def test_host_build_of_the_kernel_text_equals_the_reference(tmp_path, flags):
    exe = str(tmp_path / "rans_filter_host")
    subprocess.check_call([os.environ.get("CXX", "g++")] + flags + ["-std=c++17", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(ROOT, "r-pcc_amd", "csrc_rans"), os.path.join(ROOT, "tests", "rans_filter_host_main.cpp"), "-o", exe])
    rows = _rows()
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<q", len(rows)))
        for _, op, head, body in rows:
            f.write(struct.pack("<q%dq" % len(head), op, *head) + body)
    subprocess.check_call([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    got = open(tmp_path / "out.bin", "rb").read()
    pos = coded = 0
    for name, op, head, body in rows:
        if op == 0:
            (n,) = struct.unpack_from("<q", got, pos)
            want = C.reference(name) if head[3] else C.forced()[name][0]
            assert got[pos + 8: pos + 8 + n] == want, (name, head)
            coded += want[:2] == b"RB" and bool(head[3])
            pos += 8 + n
        else:
            st, n = struct.unpack_from("<qq", got, pos)
            pos += 16
            want_st, want = F.decode(body, cap=head[1])
            assert (st, n) == (want_st, len(want)), (name, F.NAMES.get(st, st), F.NAMES[want_st])
            if st == F.OK:
                assert got[pos: pos + n] == want, name
                pos += n
    assert pos == len(got)
    assert coded >= 60           # the encoder's coded path, with the fallback on
