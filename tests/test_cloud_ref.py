"""CPU: the cloud packer's specification (tests/cloud_ref.py) against the package's host rule over the concatenated points; librpcc_cloud.so
builds, exports what its header declares and refuses bad arguments; the tool takes --device_trailers; BatchDecompressor(device_trailers=True)
constructs with the stated bounds.  No GPU needed."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import cloud_cases as CC  # noqa: E402
import cloud_ref as C  # noqa: E402
import rows_cases as RC  # noqa: E402
import rows_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    import rpcc_amd  # noqa: F401
    from rpcc_amd import _cloud_lib
    return _cloud_lib


def _host(pc, w, extra, count):
    """The per-frame path: decode_frame's points [P + m, 3], point_intensity's fourth column, rows.pack_host."""
    from rpcc_amd import rows
    from rpcc_amd.tools.decompress import point_intensity
    pts = np.concatenate([pc, extra[: C.clamp(count, extra.shape[0])]])
    return rows.pack_host(pts, None if w is None else point_intensity(w, pts))


@pytest.mark.parametrize("with_w", [False, True])
def test_hostile_table_in_both_segments(built, with_w):
    pc, w = RC.hostile_pc(), RC.hostile_w() if with_w else None
    extra = np.concatenate([RC.hostile_pc()[::-1], np.full((3, 3), CC.POISON, np.float32)])      # the table reversed, then points past the count
    n = len(RC.HOSTILE)
    rows = C.pack(pc, w, extra, n)
    kept = int(RC.hostile_kept().sum())
    assert rows.dtype == np.float32 and rows.shape == (2 * kept, 4)
    assert rows.tobytes() == _host(pc, w, extra, n).tobytes()
    # bits unchanged in both segments; the extra rows' fourth column is +0.0 whatever the pixels carry
    assert np.array_equal(rows.view(np.uint32)[:kept, :3], pc.view(np.uint32)[RC.hostile_kept()])
    assert np.array_equal(rows.view(np.uint32)[kept:, :3], extra[:n].view(np.uint32)[RC.hostile_kept()[::-1]])
    assert not rows.view(np.uint32)[kept:, 3].any()
    if with_w:
        assert np.array_equal(rows.view(np.uint32)[:kept, 3], w.view(np.uint32)[RC.hostile_kept()])
    else:
        assert not rows.view(np.uint32)[:, 3].any()
    # the count is clamped: above the capacity every point counts (the poison too), below zero none
    assert C.pack(pc, w, extra, 10 ** 6).shape[0] == 2 * kept + 3 and C.pack(pc, w, extra, -7).tobytes() == R.pack(pc, w).tobytes()
    assert C.pack(pc, w, extra, 10 ** 6).tobytes() == _host(pc, w, extra, 10 ** 6).tobytes()
    assert C.pack(pc, w).tobytes() == R.pack(pc, w).tobytes()


@pytest.mark.parametrize("pattern", CC.EXTRA_PATTERNS)
def test_batch_rule_equals_the_host_rule(built, pattern):
    B, P, cap = 3, 300, 70
    for kind in ("zero", "one", "full", "above", "negative", "half"):
        pc, w, ri = RC.batch(B, P, "mixed", boundaries=(256,))
        counts = CC.counts_for(B, cap, kind)
        extra = CC.extras(B, cap, pattern, counts, boundaries=(32,))
        offsets, rows, nonzero = C.pack_batch(pc, w, ri, extra, counts)
        assert offsets[0] == 0 and offsets[-1] == rows.shape[0]
        for b in range(B):
            assert rows[offsets[b]: offsets[b + 1]].tobytes() == _host(pc[b], w[b], extra[b], counts[b]).tobytes(), (kind, b)
            assert nonzero[b] == (ri[b] != 0).sum()
        heads = np.diff(R.pack_batch(pc, w, ri)[0])
        tails = np.diff(offsets) - heads
        n = [C.clamp(c, cap) for c in counts]
        if pattern == "all_kept":
            assert tails.tolist() == n
        if pattern == "none_kept":
            assert tails.tolist() == [0] * B
    # no extra segment: rows_ref's batch
    a, b = C.pack_batch(pc, w, ri), R.pack_batch(pc, w, ri)
    assert a[0].tolist() == b[0].tolist() and a[1].tobytes() == b[1].tobytes()
    assert C.pack_batch(pc, w, ri, base=11)[0].tolist() == (b[0] + 11).tolist()


def test_header_symbols_exported(built):
    hdr = open(os.path.join(ROOT, "include", "rpcc_cloud.h")).read()
    declared = sorted(set(re.findall(r"\b(rpcc_cloud_[a-z0-9_]+)\s*\(", hdr)))
    assert declared == ["rpcc_cloud_last_error", "rpcc_cloud_pack", "rpcc_cloud_version"]
    lib = ctypes.CDLL(built.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    assert built.exported_symbols() == declared
    assert int(re.search(r"#define RPCC_CLOUD_ABI_VERSION (\d+)", hdr).group(1)) == built.ABI_VERSION == 1
    assert built.lib().rpcc_cloud_version() == built.ABI_VERSION
    for name, val in (("RPCC_CLOUD_MAX_BATCH", built.MAX_BATCH), ("RPCC_CLOUD_ROUND", built.ROUND), ("RPCC_CLOUD_OK", built.OK),
                      ("RPCC_CLOUD_E_CAPACITY", built.E_CAPACITY)):
        assert int(re.search(r"#define %s \(?(-?\d+)\)?" % name, hdr).group(1)) == val, name
    assert built.MAX_PIXELS == 1 << 26 and "#define RPCC_CLOUD_MAX_PIXELS (1 << 26)" in hdr
    assert built.table_words(5) == 12
    src = open(os.path.join(ROOT, "r-pcc_amd", "csrc_cloud", "cloud_kernels.hip")).read()
    threads, ppt = (int(re.search(r"#define %s (\d+)" % n, src).group(1)) for n in ("CLOUD_THREADS", "CLOUD_PPT"))
    assert threads % 64 == 0 and threads * ppt == built.ROUND
    # the table and the round are the row packer's: a caller may hand either library the same buffers
    from rpcc_amd import _rows_lib
    assert built.ROUND == _rows_lib.ROUND and built.table_words(7) == _rows_lib.table_words(7)


def test_argument_errors_do_not_crash(built):
    lib = built.lib()
    raw = ctypes.create_string_buffer(1024 + 64)     # host memory: every call below must refuse before touching it
    base = (ctypes.addressof(raw) + 63) // 64 * 64
    fill = bytes(range(256)) * 4 + b"\0" * 64
    ctypes.memmove(raw, fill, len(fill))
    pc, w, ri, rows, offs, nz, ex, cnt = base, base + 128, base + 192, base + 256, base + 512, base + 640, base + 704, base + 832

    def call(pc=pc, w=w, ri=ri, B=2, P=4, rows=rows, cap=8, offs=offs, nz=nz, start=None, ex=ex, ecap=2, cnt=cnt):
        return lib.rpcc_cloud_pack(pc, w, ri, B, P, rows, cap, offs, nz, start, ex, ecap, cnt, None)
    for bad in (dict(pc=None), dict(offs=None), dict(rows=None), dict(B=0), dict(B=-1), dict(B=65536), dict(P=0), dict(P=-3),
                dict(P=(1 << 26) + 1), dict(B=32, P=1 << 26), dict(B=2048, P=1 << 20), dict(cap=-1),
                dict(rows=rows + 8), dict(rows=rows + 4), dict(rows=rows + 1),            # rows must be 16-byte aligned
                dict(offs=offs + 4), dict(pc=pc + 2), dict(w=w + 1), dict(ri=ri + 2), dict(nz=nz + 2), dict(start=offs + 4),
                dict(ri=None),                                                            # nonzero needs ri_rec
                dict(ecap=-1), dict(ecap=(1 << 26) + 1), dict(cnt=None),                  # extra without extra_count
                dict(ex=ex + 2), dict(cnt=cnt + 1),
                dict(B=2048, P=1 << 19, ecap=1 << 19), dict(B=16, P=1 << 26, ecap=1 << 26),      # B * (P + extra_capacity) >= 2^31
                dict(B=2048, P=1 << 19, ecap=1 << 19, ex=None, cnt=None)):                # ... with or without an extra segment
        assert call(**bad) == -1, bad
        assert b"bad argument" in lib.rpcc_cloud_last_error(), bad
    assert raw.raw == fill


def test_source_digest_unchanged_by_the_cloud_library(built):
    from rpcc_amd import build as b
    before, deps = b.source_digest(), list(b.DEPS)
    b.build_cloud(force=True)
    assert b.source_digest() == before and b.DEPS == deps
    assert not any("csrc_cloud" in d or d.endswith("rpcc_cloud.h") for d in b.DEPS)
    assert os.path.exists(b.CLOUD_LIB)
    here = os.path.dirname(b.__file__)
    assert os.path.join(here, "csrc_cloud", "cloud_kernels.hip") in b.CLOUD_DEPS
    assert os.path.join(here, "csrc_tile", "tiles.h") in b.CLOUD_DEPS
    assert os.path.join(ROOT, "include", "rpcc_cloud.h") in b.CLOUD_DEPS
    assert not any("csrc_cloud" in d or d.endswith("rpcc_cloud.h") for d in b.ROWS_DEPS)      # the row packer does not depend on it


def test_front_end_names_the_missing_gpu(built):
    import torch
    from rpcc_amd import cloud
    from rpcc_amd._lib import RpccError
    with pytest.raises(RpccError, match="needs a GPU tensor"):
        cloud.pack(torch.zeros((1, 4, 3)), extra=torch.zeros((1, 2, 3)), extra_count=torch.zeros((1,), dtype=torch.int32))
    with pytest.raises(RpccError, match="needs a GPU tensor"):
        cloud.pack(np.zeros((1, 4, 3), np.float32))


def test_parser_takes_device_trailers():
    import rpcc_amd  # noqa: F401
    from rpcc_amd.tools import compress as tc
    p = tc.make_parser(datalist=True)
    assert p.parse_args([]).device_trailers is False
    on = p.parse_args(["--stream_decode", "--device_trailers"])
    assert on.device_trailers is True and on.batch_decode is True
    assert p.parse_args(["--device_trailers"]).batch_decode is False
    with pytest.raises(SystemExit):
        tc.make_parser().parse_args(["--device_trailers"])      # the single-frame tools have no such flag


@pytest.mark.parametrize("flag", ["--batch_decode", "--stream_decode"])
def test_the_flag_lifts_the_tool_s_two_refusals(built, tmp_path, flag):
    """With --device_trailers the tool gets past the --subpixel and --hidden_points refusals and fails later: where a device is needed, or,
    on a machine that has one, at the file the list names and nobody wrote."""
    from rpcc_amd.tools import compress as tc
    from rpcc_amd.tools import decompress_datalist as tdd
    lst = tmp_path / "list.txt"
    lst.write_text(str(tmp_path / "missing.rpcc") + "\n")
    base = ["--datalist", str(lst), "--output_dir", str(tmp_path / "out"), "--lidar", "Velodyne64E", flag, "--subpixel", "2", "--hidden_points"]
    with pytest.raises(NotImplementedError, match="--%s with --subpixel.*--device_trailers" % flag[2:]):
        tdd.decompress(tc.make_parser(datalist=True).parse_args(base))
    with pytest.raises(NotImplementedError, match="--%s with --hidden_points.*--device_trailers" % flag[2:]):
        tdd.decompress(tc.make_parser(datalist=True).parse_args([a for a in base if a not in ("--subpixel", "2")]))
    with pytest.raises(Exception) as err:
        tdd.decompress(tc.make_parser(datalist=True).parse_args(base + ["--device_trailers"]))
    assert not isinstance(err.value, NotImplementedError), err.value
    assert not os.path.exists(tmp_path / "out")


def test_batch_decompressor_constructs_with_the_flag(built):
    from rpcc_amd import compress_utils as cu
    from rpcc_amd.loader import StreamingDecompressor
    from rpcc_amd.pipeline import STREAM_TEXT, BatchDecompressor
    from rpcc_amd.transformer import PCTransformer
    cfg = os.path.join(ROOT, "r-pcc_amd", "lidar_cfg")
    yaml_, csv_ = os.path.join(cfg, "Velodyne_HDL_64E.yaml"), os.path.join(cfg, "Velodyne_HDL_64E_beams.csv")
    T, E = PCTransformer(yaml_, csv_, device="cpu"), PCTransformer(yaml_, device="cpu")
    P = E.H * E.W
    bd = BatchDecompressor(E, 100, 0.04, subpixel=True, hidden_points=True, device_trailers=True)
    assert bd.chunk >= 1 and bd.trailers == ("subpixel", "hidden_points") and bd.hidden_capacity == P
    assert bd.trailer_caps["subpixel"] == 8 + 2 * P == cu.SCHEMA[6].bound(P, 102) and cu.SCHEMA[6].name == "subpixel"
    assert bd.trailer_caps["hidden_points"] == 16 + P + 4 * P == cu.HIDDEN_COLUMN.bound(P, 102, P)
    small = BatchDecompressor(E, 100, 0.04, intensity=True, hidden_points=True, device_trailers=True, hidden_capacity=1000)
    assert small.trailers == ("intensity", "hidden_points") and small.trailer_caps["hidden_points"] == 16 + P + 4000
    assert small.trailer_caps["intensity"] == 8 + P and small.hidden_capacity == 1000
    # _frame_bytes counts the new arrays, so the chunk still respects the budget
    plain = BatchDecompressor(E, 100, 0.04)
    assert bd._frame_bytes() >= plain._frame_bytes() + 2 * (8 + 2 * P) + 2 * (16 + 5 * P) + 12 * P
    assert small._frame_bytes() < bd._frame_bytes() and bd.chunk * bd._frame_bytes() <= bd.CHUNK_BUDGET_BYTES

    class Tight(BatchDecompressor):
        CHUNK_BUDGET_BYTES = 3 * bd._frame_bytes()
    assert Tight(E, 100, 0.04, subpixel=True, hidden_points=True, device_trailers=True).chunk == 3
    assert Tight(E, 100, 0.04).chunk > 3
    # the flag alone changes nothing; without it the refusals stand and name it
    off = BatchDecompressor(E, 100, 0.04, device_trailers=True)
    assert off.trailers == () and off.hidden_capacity == 0 and off._frame_bytes() == plain._frame_bytes() and off.chunk == plain.chunk
    with pytest.raises(NotImplementedError, match="BatchDecompressor: subpixel.*device_trailers"):
        BatchDecompressor(E, 100, 0.04, subpixel=True)
    with pytest.raises(NotImplementedError, match="BatchDecompressor: hidden_points.*device_trailers"):
        BatchDecompressor(E, 100, 0.04, hidden_points=True)
    with pytest.raises(ValueError, match="hidden_capacity"):
        BatchDecompressor(E, 100, 0.04, hidden_points=True, device_trailers=True, hidden_capacity=-1)
    # a per-beam elevation table: what subpixel_tables() raises
    with pytest.raises(NotImplementedError, match="subpixel with a per-beam elevation table"):
        BatchDecompressor(T, 100, 0.04, subpixel=True, device_trailers=True)
    # the streaming front end follows its decompressor
    with pytest.raises(NotImplementedError, match="StreamingDecompressor: hidden_points.*device_trailers"):
        StreamingDecompressor(plain, hidden_points=True)
    with pytest.raises(NotImplementedError, match="StreamingDecompressor: hidden_points"):
        StreamingDecompressor(BatchDecompressor(E, 100, 0.04, subpixel=True, device_trailers=True), hidden_points=True)
    from rpcc_amd import _lib
    assert "subpixel" in STREAM_TEXT[_lib.STREAM_E_SUBPIXEL] and "hidden_points" in STREAM_TEXT[_lib.STREAM_E_HIDDEN]
    assert (_lib.STREAM_E_SUBPIXEL, _lib.STREAM_E_HIDDEN) == (11, 12)
