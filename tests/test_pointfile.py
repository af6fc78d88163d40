"""rpcc_amd/pointfile.py on the table of tests/pointfile_cases.py: every accepted file gives the rows it was made of, bit for bit, from its
bytes and from a file on disk; every refused file raises ValueError naming the file and the reason.  The layouts of the named cases, the
round trips of what save_point_cloud_to_file writes, write_pcd's header, and librpcc_host.so's LZF decoder against tests/lzf_ref.py.
No GPU needed."""
import ctypes
import os

import numpy as np
import pytest

import lzf_ref as Z
import pointfile_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pf():
    import __graft_entry__ as ge
    ge.build()
    from rpcc_amd import pointfile
    return pointfile


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_the_table_holds_what_the_specification_names():
    names = [c[0] for c in PC.CASES]
    assert len(set(names)) == len(names) and len(PC.ACCEPTED) >= 20 and len(PC.REFUSED) >= 15
    assert all(c[3].dtype == np.float32 and c[3].ndim == 2 and c[3].shape[1] == 4 for c in PC.ACCEPTED)


@pytest.mark.parametrize("case", PC.ACCEPTED, ids=[c[0] for c in PC.ACCEPTED])
def test_accepted(pf, case, tmp_path):
    name, fmt, data, want = case
    got = pf.read_rows(data, name=name, fmt=fmt)
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(bits(got), bits(want)), name
    path = tmp_path / ("f." + fmt)
    path.write_bytes(data)
    assert np.array_equal(bits(pf.read_rows(str(path))), bits(want))
    lay = pf.read_layout(str(path))
    assert lay.n == want.shape[0] and lay.fmt == fmt
    assert data[lay.data_off - 1: lay.data_off] == b"\n" and data[:lay.data_off].rstrip().endswith((b"end_header", b"ascii", b"binary", b"binary_compressed"))


@pytest.mark.parametrize("case", PC.REFUSED, ids=[c[0] for c in PC.REFUSED])
def test_refused(pf, case, tmp_path):
    name, fmt, data, why = case
    path = tmp_path / (name + "." + fmt)
    path.write_bytes(data)
    with pytest.raises(ValueError) as e:
        pf.read_rows(str(path))
    assert why in str(e.value) and str(path) in str(e.value), str(e.value)
    with pytest.raises(ValueError) as e:
        pf.read_rows(data, name="given-name", fmt=fmt)
    assert why in str(e.value) and "given-name" in str(e.value)


def layout_of(pf, name):
    c = [c for c in PC.CASES if c[0] == name][0]
    return pf.read_layout(c[2], name=name, fmt=c[1]), c


def test_layouts(pf):
    F32, NONE = pf.F32, pf.NONE
    lay, _ = layout_of(pf, "xyz_f32_step12")
    assert (lay.off, lay.step, lay.type, lay.data, lay.body_bytes) == ([0, 4, 8, 0], [12, 12, 12, 0], [F32, F32, F32, NONE], "binary", 12 * 37)
    assert not lay.has_intensity
    lay, _ = layout_of(pf, "xyzi_f32_step16")
    assert (lay.off, lay.step, lay.type) == ([0, 4, 8, 12], [16] * 4, [F32] * 4) and lay.has_intensity
    st = pf.stored_layout(37)
    assert (st.off, st.step, st.type, st.body_bytes) == (lay.off, lay.step, lay.type, lay.body_bytes)
    lay, _ = layout_of(pf, "pcl_pointxyzi_step32")
    assert (lay.off, lay.step, lay.type) == ([0, 4, 8, 16], [32] * 4, [F32] * 4)
    lay, c = layout_of(pf, "velodyne_step22_odd_header")
    assert (lay.off, lay.step) == ([0, 4, 8, 12], [22] * 4) and lay.data_off % 2 == 1 and lay.data_off == len(c[2]) - 22 * 37
    lay, _ = layout_of(pf, "fields_z_y_x")
    assert lay.off == [8, 4, 0, 0] and lay.type[3] == NONE
    lay, _ = layout_of(pf, "intensity_i16_negative")
    assert (lay.off, lay.step, lay.type) == ([0, 4, 8, 12], [14] * 4, [F32, F32, F32, pf.I16])
    lay, _ = layout_of(pf, "f64_rounding")
    assert (lay.off, lay.step, lay.type) == ([0, 8, 16, 24], [32] * 4, [pf.F64] * 4)
    lay, _ = layout_of(pf, "organised_height_64")
    assert lay.n == 192
    # planes: FIELDS x _ y normal z intensity, SIZE 4 1 4 4 4 2, COUNT 1 4 1 3 1 1, 300 points
    lay, _ = layout_of(pf, "binary_compressed_planes")
    assert (lay.off, lay.step, lay.type) == ([0, 300 * 8, 300 * 24, 300 * 28], [4, 4, 4, 2], [F32, F32, F32, pf.U16])
    assert lay.data == "binary_compressed" and lay.body_bytes == 300 * 30
    lay, _ = layout_of(pf, "ply_short_names_face_after_vertex")
    assert (lay.off, lay.step, lay.type) == ([0, 4, 8, 12], [21] * 4, [F32, F32, F32, pf.U8])
    d = lay.desc(1000)
    assert d.dtype == np.int64 and d.tolist() == [1000, 21 * 37, 37, 0, 4, 8, 12, 21, 21, 21, 21, F32, F32, F32, pf.U8, 0]
    assert pf.DESC_WORDS == 16 and pf.TYPE_SIZE == (0, 4, 8, 1, 1, 2, 2, 4, 4)
    assert pf.is_point_file("a/b.pcd") and pf.is_point_file("c.ply") and not pf.is_point_file("c.bin")


def test_round_trips_of_what_the_package_writes(pf, tmp_path):
    from rpcc_amd.dataset import DatasetTemplate as D
    rng = np.random.default_rng(8)
    pts = rng.uniform(-50, 50, (200, 3)).astype(np.float32)
    pts[5] = 0                                  # dropped by the sum != 0 filter
    pts[6] = (1.5, -1.5, 0)                     # and so is this one
    w = rng.uniform(0, 1, 200).astype(np.float32)
    keep = pts.sum(-1) != 0
    assert keep.sum() == 198
    for ext in ("ply", "pcd"):
        D.save_point_cloud_to_file(str(tmp_path / ("a." + ext)), pts, intensity=w)
        D.save_point_cloud_to_file(str(tmp_path / ("b." + ext)), pts)
        rows = pf.read_rows(str(tmp_path / ("a." + ext)))
        assert np.array_equal(bits(rows), bits(np.concatenate([pts[keep], w[keep, None]], 1)))
        assert np.array_equal(bits(D.load_rows(str(tmp_path / ("a." + ext)))), bits(rows))
        assert np.array_equal(bits(D.load_data(str(tmp_path / ("a." + ext)))), bits(pts[keep]))
        rows = D.load_rows(str(tmp_path / ("b." + ext)))
        assert np.array_equal(bits(rows[:, :3]), bits(pts[keep])) and not bits(rows[:, 3]).any()      # no intensity in the file: +0.0
        assert not pf.read_layout(str(tmp_path / ("b." + ext))).has_intensity


def test_write_pcd_header(pf, tmp_path):
    pts = np.arange(15, dtype=np.float64).reshape(5, 3)
    pf.write_pcd(str(tmp_path / "a.pcd"), pts, intensity=np.arange(5))
    raw = (tmp_path / "a.pcd").read_bytes()
    head = (b"# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z intensity\nSIZE 4 4 4 4\nTYPE F F F F\nCOUNT 1 1 1 1\n"
            b"WIDTH 5\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS 5\nDATA binary\n")
    assert raw[:len(head)] == head == pf.pcd_header(5, True) and len(raw) == len(head) + 5 * 16
    assert np.array_equal(np.frombuffer(raw[len(head):], "<f4").reshape(5, 4), np.concatenate([pts, np.arange(5)[:, None]], 1).astype(np.float32))
    pf.write_pcd(str(tmp_path / "b.pcd"), pts)
    raw = (tmp_path / "b.pcd").read_bytes()
    head = (b"# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z\nSIZE 4 4 4\nTYPE F F F\nCOUNT 1 1 1\n"
            b"WIDTH 5\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS 5\nDATA binary\n")
    assert raw[:len(head)] == head and len(raw) == len(head) + 5 * 12
    with pytest.raises(ValueError, match="intensities"):
        pf.write_pcd(str(tmp_path / "c.pcd"), pts, intensity=np.arange(4))


# ---- LZF ---------------------------------------------------------------------------------------------------------------------------------
def lzf_streams():
    rng = np.random.default_rng(77)
    noise = rng.integers(0, 256, 9000, dtype=np.uint8).tobytes()
    S = {}
    S["literal_run_over_32"] = (Z.literals(noise[:100]), noise[:100])
    S["match_2_plus_7"] = (Z.literals(noise[:20]) + Z.match(9, 20), noise[:20] + noise[:9])
    S["match_2_plus_7_plus_255"] = (Z.literals(noise[:300]) + Z.match(264, 300), noise[:300] + noise[:264])
    S["distance_8192"] = (Z.literals(noise[:8192]) + Z.match(5, 8192) + Z.match(3, 1), noise[:8192] + noise[:5] + noise[4:5] * 3)
    S["distance_1_overlapping_run"] = (Z.literals(b"ab") + Z.match(200, 1), b"a" + b"b" * 201)
    S["overlap_distance_3"] = (Z.literals(b"xyz") + Z.match(10, 3), b"xyz" + b"xyzxyzxyzx")
    S["empty"] = (b"", b"")
    text = (b"0123456789" * 50 + noise[:500]) * 3
    S["greedy_encoder"] = (Z.encode(text), text)
    return S


def host_decode(pf, src, size, slack=64):
    """-> (status, bytes written, the size bytes, the slack bytes behind them) through librpcc_host.so."""
    from rpcc_amd import _lib
    buf = np.full(size + slack, 0xA5, np.uint8)
    s = np.frombuffer(src, np.uint8)
    got = ctypes.c_size_t(0)
    rc = _lib.host_lib().rpcc_lzf_decompress(s.ctypes.data if s.size else None, s.size, buf.ctypes.data, size, ctypes.byref(got))
    return rc, got.value, buf[:size].tobytes(), buf[size:].tobytes()


@pytest.mark.parametrize("name", sorted(lzf_streams()))
def test_lzf_streams_decode_to_their_source(pf, name):
    src, want = lzf_streams()[name]
    assert Z.decode(src, len(want)) == (Z.OK, want)
    rc, got, out, slack = host_decode(pf, src, len(want))
    assert (rc, got, out) == (0, len(want), want) and slack == b"\xa5" * 64
    dst = np.empty(len(want), np.uint8)
    assert pf.lzf_decompress(src, dst).tobytes() == want
    if name == "greedy_encoder":
        assert len(src) < len(want) // 2


def test_lzf_refusals_write_nothing_past_the_stated_size(pf):
    S = lzf_streams()
    src, want = S["match_2_plus_7_plus_255"]
    cases = [(src[:-1], len(want), Z.E_TRUNCATED), (src[:-2], len(want), Z.E_TRUNCATED), (Z.literals(want[:40])[:-1], 40, Z.E_TRUNCATED), (bytes([0xE0]), 8, Z.E_TRUNCATED),
             (Z.match(3, 1), 8, Z.E_DISTANCE), (Z.literals(b"abcd") + Z.match(3, 5), 8, Z.E_DISTANCE),
             (src, len(want) - 1, Z.E_OVERFLOW), (src, 300, Z.E_OVERFLOW), (Z.literals(want[:40]), 39, Z.E_OVERFLOW), (S["distance_1_overlapping_run"][0], 100, Z.E_OVERFLOW),
             (src, 0, Z.E_OVERFLOW)]
    for stream, size, status in cases:
        st, before = Z.decode(stream, size)
        assert st == status
        rc, got, out, slack = host_decode(pf, stream, size)
        assert rc == status and got == len(before) and out[:got] == before, (stream[:8], size)
        assert out[got:] == b"\xa5" * (size - got) and slack == b"\xa5" * 64
        with pytest.raises(ValueError, match="LZF"):
            pf.lzf_decompress(stream, np.empty(size, np.uint8), "x.pcd")
    with pytest.raises(ValueError, match="decodes to 20 bytes, the header states 21"):
        pf.lzf_decompress(Z.literals(want[:20]), np.empty(21, np.uint8))
    from rpcc_amd import _lib
    assert _lib.host_lib().rpcc_lzf_decompress(None, 4, None, 0, None) == -1


def test_host_header_declares_the_decoder():
    hdr = open(os.path.join(ROOT, "include", "rpcc_host.h")).read()
    assert "int rpcc_lzf_decompress(const uint8_t *src, size_t src_bytes, uint8_t *dst, size_t dst_bytes, size_t *out_bytes);" in hdr
    from rpcc_amd import build as b
    assert b.HOST_LZF_SRC not in b.DEPS and not any("csrc_fields" in d for d in b.DEPS)
