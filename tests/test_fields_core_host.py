"""csrc_fields/fields_rule.h and csrc_fields/lzf_decode.h, the text the gfx950 unpack kernel and librpcc_host.so are compiled from, built
for the host (tests/fields_host_main.cpp) and run over the table of tests/pointfile_cases.py, over refused descriptors and over the LZF
streams of tests/test_pointfile.py: plain, and with -fsanitize=address,undefined, the runtimes inside the program.  No GPU needed."""
import os
import struct
import subprocess

import numpy as np
import pytest

import fields_ref as FR
import lzf_ref as Z
import pointfile_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = {"plain": ["-O2", "-ffp-contract=off"],
          "sanitized": ["-O1", "-ffp-contract=off", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]}


@pytest.fixture(scope="module", params=sorted(BUILDS))
def exe(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fields_host_" + request.param) / "fields_host")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17"] + BUILDS[request.param] +
                          ["-I", os.path.join(ROOT, "r-pcc_amd", "csrc_fields"), os.path.join(ROOT, "tests", "fields_host_main.cpp"), "-o", out])
    return out


@pytest.fixture(scope="module")
def pf():
    import rpcc_amd  # noqa: F401
    from rpcc_amd import pointfile
    return pointfile


def run_unpack(exe, tmp_path, chunk, desc, offs):
    B, total = desc.shape[0], int(offs[-1])
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<3q", chunk.size, B, total) + desc.astype("<i8").tobytes() + offs.astype("<i8").tobytes() + chunk.tobytes())
    run = subprocess.run([exe, "unpack", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], stderr=subprocess.PIPE)
    assert run.returncode == 0 and not run.stderr, run.stderr.decode(errors="replace")[-4000:]
    raw = (tmp_path / "out.bin").read_bytes()
    assert len(raw) == 16 * total + 4 * B
    return np.frombuffer(raw[:16 * total], np.uint32).reshape(-1, 4), np.frombuffer(raw[16 * total:], np.int32)


def test_the_table(exe, pf, tmp_path):
    frames = [FR.case_frame(pf, c) for c in PC.ACCEPTED]
    for kw in (dict(), dict(lead=3), dict(abut=True)):
        chunk, desc, offs, want = FR.build_chunk(frames, **kw)
        rows, status = run_unpack(exe, tmp_path, chunk, desc, offs)
        assert not status.any()
        assert np.array_equal(rows, want.view(np.uint32)), kw


def test_refused_descriptors(exe, pf, tmp_path):
    """One good frame between refused ones: E_LAYOUT and +0.0 rows for those, the good frame's rows for it.  Every byte a refused descriptor
    names by off and step still lies inside the chunk, so that a program that did read it would read the chunk's own bytes."""
    rng = np.random.default_rng(3)
    good = FR.record_frame(rng, 50, 22)
    bad = []
    for edit in (lambda d: d.__setitem__(3 + 2, d[3 + 2] + 12),         # z's range ends 2 bytes past the span
                 lambda d: d.__setitem__(7 + 0, 3),                     # a step below the size
                 lambda d: d.__setitem__(7 + 1, 257),                   # a step above RPCC_FIELDS_MAX_STEP
                 lambda d: d.__setitem__(2, 49),                        # a row count that disagrees (see below: the rows stay 50)
                 lambda d: d.__setitem__(11 + 1, 0),                    # no y
                 lambda d: d.__setitem__(11 + 3, 9),                    # an unknown type
                 lambda d: d.__setitem__(3 + 1, -1),                    # a negative offset
                 lambda d: d.__setitem__(1, 49 * 22 + 15)):             # a span one byte short of the last intensity
        data, d, want = FR.record_frame(rng, 50, 22)
        d = d.copy()
        edit(d)
        bad.append((data + bytes(300 * 50), d, np.zeros((50, 4), np.float32)))      # (room behind the records for the widest step)
    frames = bad[:4] + [good] + bad[4:]
    chunk, desc, offs, want = FR.build_chunk(frames)
    rows, status = run_unpack(exe, tmp_path, chunk, desc, offs)
    assert status.tolist() == [FR.E_LAYOUT] * 4 + [FR.OK] + [FR.E_LAYOUT] * 4
    assert np.array_equal(rows, want.view(np.uint32))
    # spans outside the chunk, and a row range outside 0 .. total: no row of such a frame is written (the program pre-fills with 0xA5)
    d1, d2 = good[1].copy(), good[1].copy()
    d1[0], d2[1] = len(good[0]) + 1, len(good[0]) + 1
    for d in (d1, d2):
        rows, status = run_unpack(exe, tmp_path, np.frombuffer(good[0], np.uint8), d[None], np.array([0, 50], np.int64))
        assert status.tolist() == [FR.E_LAYOUT] and not rows.any()
    rows, status = run_unpack(exe, tmp_path, np.frombuffer(good[0], np.uint8), np.stack([good[1], good[1]]), np.array([0, 60, 50], np.int64))
    assert status.tolist() == [FR.E_LAYOUT, FR.E_LAYOUT] and (rows == 0xA5A5A5A5).all()


def test_every_type_at_every_alignment(exe, tmp_path):
    rng = np.random.default_rng(4)
    frames = []
    for t in range(1, 9):
        for lead in range(4):
            data, d, want = FR.record_frame(rng, 9, 31, types=(t, FR.F32, t, t))
            frames.append((data, d, want))
    for lead in range(4):
        chunk, desc, offs, want = FR.build_chunk(frames, lead=lead)
        rows, status = run_unpack(exe, tmp_path, chunk, desc, offs)
        assert not status.any() and np.array_equal(rows, want.view(np.uint32))


def test_lzf(exe, tmp_path):
    from test_pointfile import lzf_streams
    S = lzf_streams()

    def run(stream, size):
        (tmp_path / "s.lzf").write_bytes(stream)
        r = subprocess.run([exe, "lzf", str(tmp_path / "s.lzf"), str(tmp_path / "s.out"), str(size)], stderr=subprocess.PIPE)
        assert r.returncode == 0 and not r.stderr, r.stderr.decode(errors="replace")[-4000:]
        raw = (tmp_path / "s.out").read_bytes()
        rc, got = struct.unpack("<iq", raw[:12])
        assert len(raw) == 12 + size
        return rc, got, raw[12:]

    for name, (stream, want) in S.items():
        assert run(stream, len(want)) == (0, len(want), want), name
    src, want = S["match_2_plus_7_plus_255"]
    for stream, size in ((src[:-1], len(want)), (Z.match(3, 1), 8), (Z.literals(b"abcd") + Z.match(3, 5), 8), (src, len(want) - 1), (src, 0),
                         (S["distance_1_overlapping_run"][0], 100), (bytes([0xE0]), 8), (bytes([0xFF, 0xFF]), 8)):
        st, before = Z.decode(stream, size)
        assert st != Z.OK
        rc, got, out = run(stream, size)
        assert (rc, got) == (st, len(before)) and out == before + b"\xa5" * (size - got)
