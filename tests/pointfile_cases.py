"""One table of .pcd / .ply files for rpcc_amd/pointfile.py, the host build of csrc_fields/fields_rule.h and the gfx950 kernel:
CASES = [(name, fmt, file bytes, expected)], expected = the float32 [n,4] rows, built from the arrays the file was made of and never through
the reader, or the text a ValueError must hold.  tests/test_pointfile.py runs it on the host reader, tests/test_fields_core_host.py on the
host program, tests/test_gpu_fields.py on the device.  No GPU."""
import struct

import numpy as np

import lzf_ref as Z

F4, F8 = "<f4", "<f8"


def f32(bits):
    return np.array(bits, dtype=np.uint32).view(np.float32)


def rows_of(x, y, z, w=None):
    """Expected rows from float32 columns (bit copies)."""
    out = np.zeros((len(x), 4), np.uint32)
    for c, col in enumerate((x, y, z, w)):
        if col is not None:
            out[:, c] = np.asarray(col, dtype=np.float32).view(np.uint32)
    return out.view(np.float32)


def pcd(fields, size, kind, body, n, count=None, data="binary", width=None, height=1, points=True, viewpoint=True, lead="# .PCD v0.7 - Point Cloud Data file format\n"):
    h = lead + "VERSION 0.7\nFIELDS %s\nSIZE %s\nTYPE %s\n" % (" ".join(fields), " ".join(str(s) for s in size), " ".join(kind))
    if count is not None:
        h += "COUNT %s\n" % " ".join(str(c) for c in count)
    h += "WIDTH %d\nHEIGHT %d\n" % (n // height if width is None else width, height)
    if viewpoint:
        h += "VIEWPOINT 0 0 0 1 0 0 0\n"
    if points is True:
        h += "POINTS %d\n" % n
    elif points is not False:
        h += "POINTS %d\n" % points
    return (h + "DATA %s\n" % data).encode() + body


def packed(cols):
    """[(name, dtype string or (dtype, count), values or None)] -> the array-of-structures bytes; None = padding of 0xEE bytes."""
    n = max(len(v) for _, _, v in cols if v is not None)
    dt = np.dtype([(name if name != "_" else "_%d" % i, d) if isinstance(d, str) else (name if name != "_" else "_%d" % i, d[0], (d[1],))
                   for i, (name, d, _) in enumerate(cols)])
    rec = np.zeros(n, dt)
    rec.view(np.uint8)[:] = 0xEE
    for i, (name, _, v) in enumerate(cols):
        if v is not None:
            rec[dt.names[i]] = v
    return rec.tobytes(), dt.itemsize


def planes(cols):
    """The same columns field-major: what a binary_compressed body decompresses to."""
    n = max(len(v) for _, _, v in cols if v is not None)
    out = b""
    for name, d, v in cols:
        dt, cnt = (d, 1) if isinstance(d, str) else d
        a = np.zeros((n, cnt), dt)
        a.view(np.uint8)[:] = 0xEE
        if v is not None:
            a[:, 0] = v
        out += a.tobytes()
    return out


def compressed(raw, comp=None, stated=None):
    comp = Z.encode(raw) if comp is None else comp
    return struct.pack("<II", len(comp), len(raw) if stated is None else stated) + comp


def ply(props, body, n, fmt="binary_little_endian", tail_header="", extra=""):
    h = "ply\nformat %s 1.0\ncomment made by hand\nobj_info nothing\n%selement vertex %d\n" % (fmt, extra, n)
    h += "".join("property %s %s\n" % (t, name) for t, name in props)
    return (h + tail_header + "end_header\n").encode() + body


def _cases():
    rng = np.random.default_rng(2510)
    n = 37
    x, y, z, w = (rng.uniform(-80, 80, n).astype(np.float32) for _ in range(4))
    w = np.abs(w)
    C = []

    body, step = packed([("x", F4, x), ("y", F4, y), ("z", F4, z)])
    assert step == 12
    C.append(("xyz_f32_step12", "pcd", pcd("xyz", (4, 4, 4), "FFF", body, n, count=(1, 1, 1)), rows_of(x, y, z)))

    body, step = packed([("x", F4, x), ("y", F4, y), ("z", F4, z), ("intensity", F4, w)])
    assert step == 16
    C.append(("xyzi_f32_step16", "pcd", pcd(["x", "y", "z", "intensity"], (4,) * 4, "FFFF", body, n, count=(1,) * 4), rows_of(x, y, z, w)))

    body, step = packed([("x", F4, x), ("y", F4, y), ("z", F4, z), ("_", ("u1", 4), None), ("intensity", F4, w), ("_", ("u1", 12), None)])
    assert step == 32
    C.append(("pcl_pointxyzi_step32", "pcd", pcd(["x", "y", "z", "_", "intensity", "_"], (4, 4, 4, 1, 4, 1), "FFFUFU", body, n, count=(1, 1, 1, 4, 1, 12)),
              rows_of(x, y, z, w)))

    ring, t = rng.integers(0, 16, n).astype("<u2"), rng.uniform(0, 0.1, n).astype(np.float32)
    body, step = packed([("x", F4, x), ("y", F4, y), ("z", F4, z), ("intensity", F4, w), ("ring", "<u2", ring), ("time", F4, t)])
    assert step == 22
    file = pcd(["x", "y", "z", "intensity", "ring", "time"], (4, 4, 4, 4, 2, 4), "FFFFUF", body, n, count=(1,) * 6, lead="# velodyne\n")
    if (len(file) - len(body)) % 2 == 0:
        file = pcd(["x", "y", "z", "intensity", "ring", "time"], (4, 4, 4, 4, 2, 4), "FFFFUF", body, n, count=(1,) * 6, lead="# velodyne.\n")
    assert (len(file) - len(body)) % 2 == 1       # the header's length is odd: no field is aligned
    C.append(("velodyne_step22_odd_header", "pcd", file, rows_of(x, y, z, w)))

    # F64: ties to even (1 + 2^-24 -> 1; 1 + 3 * 2^-24 -> 1 + 2^-22), overflow, a subnormal result, ties among the subnormals
    d = np.array([1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, 1e39, -1e39, 2.0 ** -140, 2.0 ** -150, 3 * 2.0 ** -150, -0.0, 0.1], np.float64)
    want = f32([0x3F800000, 0x3F800002, 0x7F800000, 0xFF800000, 0x00000200, 0x00000000, 0x00000002, 0x80000000, 0x3DCCCCCD])
    body, step = packed([("x", F8, d), ("y", F8, d[::-1]), ("z", F8, d), ("intensity", F8, d)])
    assert step == 32
    C.append(("f64_rounding", "pcd", pcd(["x", "y", "z", "intensity"], (8,) * 4, "FFFF", body, len(d)), rows_of(want, want[::-1], want, want)))

    k = 6
    for name, dt, size, kind, vals, exp in (
            ("u8", "u1", 1, "U", [0, 255, 7, 128, 1, 200], [0.0, 255.0, 7.0, 128.0, 1.0, 200.0]),
            ("i8", "i1", 1, "I", [0, -128, 127, -1, 1, 5], [0.0, -128.0, 127.0, -1.0, 1.0, 5.0]),
            ("u16", "<u2", 2, "U", [0, 65535, 256, 1, 40000, 9], [0.0, 65535.0, 256.0, 1.0, 40000.0, 9.0]),
            ("i16_negative", "<i2", 2, "I", [-32768, -1, 32767, 0, -300, 300], [-32768.0, -1.0, 32767.0, 0.0, -300.0, 300.0]),
            ("u32_16777217", "<u4", 4, "U", [16777217, 16777219, 4294967295, 0, 16777216, 3], [16777216.0, 16777220.0, 4294967296.0, 0.0, 16777216.0, 3.0]),
            ("i32_minimum", "<i4", 4, "I", [-2147483648, 2147483647, -16777217, -1, 0, 16777219], [-2147483648.0, 2147483648.0, -16777216.0, -1.0, 0.0, 16777220.0])):
        body, step = packed([("x", F4, x[:k]), ("y", F4, y[:k]), ("z", F4, z[:k]), ("intensity", dt, np.array(vals, dt))])
        assert step == 12 + size
        C.append(("intensity_" + name, "pcd", pcd(["x", "y", "z", "intensity"], (4, 4, 4, size), "FFF" + kind, body, k),
                  rows_of(x[:k], y[:k], z[:k], np.array(exp, np.float32))))

    body, _ = packed([("z", F4, z), ("y", F4, y), ("x", F4, x)])
    C.append(("fields_z_y_x", "pcd", pcd("zyx", (4, 4, 4), "FFF", body, n), rows_of(x, y, z)))

    bits = f32([0x7FC12345, 0xFF800001, 0x80000000, 0x7F800000, 0x00000001])       # NaN payloads, -0.0, inf, the smallest subnormal
    body, _ = packed([("x", F4, bits), ("y", F4, bits[::-1]), ("z", F4, bits), ("intensity", F4, bits)])
    C.append(("nan_payload_and_negative_zero", "pcd", pcd(["x", "y", "z", "intensity"], (4,) * 4, "FFFF", body, 5), rows_of(bits, bits[::-1], bits, bits)))

    body, _ = packed([("x", F4, x), ("y", F4, y), ("z", F4, z)])
    C.append(("no_count_points_viewpoint", "pcd", pcd("xyz", (4, 4, 4), "FFF", body, n, points=False, viewpoint=False), rows_of(x, y, z)))

    m = 3 * 64
    ox, oy, oz = (rng.uniform(-50, 50, m).astype(np.float32) for _ in range(3))
    body, _ = packed([("x", F4, ox), ("y", F4, oy), ("z", F4, oz)])
    C.append(("organised_height_64", "pcd", pcd("xyz", (4, 4, 4), "FFF", body, m, width=3, height=64), rows_of(ox, oy, oz)))

    C.append(("points_0", "pcd", pcd(["x", "y", "z", "intensity"], (4,) * 4, "FFFF", b"", 0, width=0), np.zeros((0, 4), np.float32)))

    text = "1.5 -2.25 3 0.5 7\n0.1 1e39 -0 255 8\nnan 2 16777217 1e-40 9\n"
    exp = rows_of(f32([0x3FC00000, 0x3DCCCCCD, 0x7FC00000]), f32([0xC0100000, 0x7F800000, 0x40000000]),
                  f32([0x40400000, 0x80000000, 0x4B800000]), f32([0x3F000000, 0x437F0000, 0x000116C2]))
    C.append(("ascii_pcd", "pcd", pcd(["x", "y", "z", "intensity", "ring"], (4, 4, 4, 4, 2), "FFFFU", text.encode(), 3, data="ascii"), exp))
    C.append(("ascii_ply", "ply", ply([("float", "x"), ("float", "y"), ("float", "z"), ("float", "intensity"), ("uchar", "ring")],
                                      (text + "3 0 1 2\n").encode(), 3, fmt="ascii", tail_header="element face 1\nproperty list uchar int vertex_indices\n"), exp))

    u8 = rng.integers(0, 256, n).astype("u1")
    body, step = packed([("x", F4, x), ("y", F4, y), ("z", F4, z), ("intensity", "u1", u8), ("nx", F8, x.astype(np.float64))])
    assert step == 21
    face = bytes([3]) + struct.pack("<3i", 0, 1, 2)
    for spell, names in (("short_names", ("float", "uchar", "double")), ("sized_names", ("float32", "uint8", "float64"))):
        props = [(names[0], "x"), (names[0], "y"), (names[0], "z"), (names[1], "intensity"), (names[2], "nx")]
        C.append(("ply_" + spell + "_face_after_vertex", "ply",
                  ply(props, body + face, n, tail_header="element face 1\nproperty list uchar int vertex_indices\n"), rows_of(x, y, z, u8.astype(np.float32))))
    body, _ = packed([("x", F4, x), ("y", F4, y), ("z", F4, z)])
    C.append(("ply_xyz", "ply", ply([("float", "x"), ("float", "y"), ("float", "z")], body, n), rows_of(x, y, z)))

    # binary_compressed: planes, a padding field and a COUNT > 1 field between the used ones; repeated values, so that the stream has matches
    cx = np.repeat(x[:8], 40)[:300]
    cy, cz, cw = np.roll(cx, 7), np.roll(cx, 11), np.repeat(np.arange(10, dtype="<u2") * 6553, 30)
    cols = [("x", F4, cx), ("_", ("u1", 4), None), ("y", F4, cy), ("normal", (F4, 3), None), ("z", F4, cz), ("intensity", "<u2", cw)]
    hdr = dict(fields=["x", "_", "y", "normal", "z", "intensity"], size=(4, 1, 4, 4, 4, 2), kind="FUFFFU", n=300, count=(1, 4, 1, 3, 1, 1), data="binary_compressed")
    raw = planes(cols)
    assert len(raw) == 300 * 30
    C.append(("binary_compressed_planes", "pcd", pcd(body=compressed(raw), **hdr), rows_of(cx, cy, cz, cw.astype(np.float32))))
    C.append(("binary_compressed_empty", "pcd", pcd(["x", "y", "z"], (4, 4, 4), "FFF", compressed(b""), 0, width=0, data="binary_compressed"), np.zeros((0, 4), np.float32)))

    # ---- refusals --------------------------------------------------------------------------------------------------------------------
    body, _ = packed([("x", F4, x), ("y", F4, y), ("z", F4, z)])
    C.append(("refuse_missing_z", "pcd", pcd(["x", "y", "k"], (4, 4, 4), "FFF", body, n), "no field z"))
    C.append(("refuse_count_on_x", "pcd", pcd(["x", "y", "z"], (2, 4, 4), "FFF", body, n, count=(2, 1, 1)), "field x has COUNT 2"))
    body8, _ = packed([("x", F4, x), ("y", F4, y), ("z", F4, z), ("intensity", "<i8", np.arange(n))])
    C.append(("refuse_size8_type_i", "pcd", pcd(["x", "y", "z", "intensity"], (4, 4, 4, 8), "FFFI", body8, n), "SIZE 8 TYPE I"))
    C.append(("refuse_size8_type_u", "pcd", pcd(["x", "y", "z", "intensity"], (4, 4, 4, 8), "FFFU", body8, n), "SIZE 8 TYPE U"))
    C.append(("refuse_size2_type_f", "pcd", pcd(["x", "y", "z"], (2, 4, 4), "FFF", body, n), "SIZE 2 TYPE F"))
    C.append(("refuse_points_not_width_height", "pcd", pcd("xyz", (4, 4, 4), "FFF", body, n, points=n - 1), "is not WIDTH * HEIGHT"))
    C.append(("refuse_short_body", "pcd", pcd("xyz", (4, 4, 4), "FFF", body[:-1], n), "the body holds"))
    C.append(("refuse_short_ascii_body", "pcd", pcd("xyz", (4, 4, 4), "FFF", b"1 2 3\n4 5\n", 2, data="ascii"), "the body holds"))
    C.append(("refuse_unknown_data", "pcd", pcd("xyz", (4, 4, 4), "FFF", body, n, data="binary_zstd"), "unknown DATA"))
    C.append(("refuse_big_endian", "ply", ply([("float", "x"), ("float", "y"), ("float", "z")], body, n, fmt="binary_big_endian"), "binary_big_endian"))
    C.append(("refuse_list_in_vertex", "ply", ply([("float", "x"), ("float", "y"), ("float", "z"), ("list uchar", "int k")], body, n), "list property"))
    C.append(("refuse_vertex_not_first", "ply", ply([("float", "x"), ("float", "y"), ("float", "z")], body, n,
                                                    extra="element face 0\nproperty list uchar int vertex_indices\n"), "vertex must be the first element"))
    C.append(("refuse_ply_missing_y", "ply", ply([("float", "x"), ("float", "k"), ("float", "z")], body, n), "no property y"))
    C.append(("refuse_ply_short_body", "ply", ply([("float", "x"), ("float", "y"), ("float", "z")], body[:-5], n), "the body holds"))
    good = Z.encode(raw)
    C.append(("refuse_lzf_truncated", "pcd", pcd(body=compressed(raw, comp=good[:-1]), **hdr), "ends inside"))
    C.append(("refuse_lzf_distance", "pcd", pcd(body=compressed(raw, comp=Z.literals(raw[:4]) + Z.match(3, 5) + good), **hdr), "before the first output byte"))
    C.append(("refuse_lzf_overflow", "pcd", pcd(body=compressed(raw, comp=good + Z.literals(b"\x01")), **hdr), "past the stated uncompressed size"))
    C.append(("refuse_lzf_short", "pcd", pcd(body=compressed(raw, comp=Z.encode(raw[:-3])), **hdr), "decodes to 8997 bytes"))
    C.append(("refuse_uncompressed_size", "pcd", pcd(body=compressed(raw, stated=len(raw) + 1), **hdr), "uncompressed_size 9001 is not"))
    C.append(("refuse_compressed_size", "pcd", pcd(body=compressed(raw)[:-1], **hdr), "compressed_size states"))
    return C


CASES = _cases()
ACCEPTED = [c for c in CASES if not isinstance(c[3], str)]
REFUSED = [c for c in CASES if isinstance(c[3], str)]
