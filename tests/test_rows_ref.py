"""CPU: the row packer's specification (tests/rows_ref.py) against the bytes DatasetTemplate.save_point_cloud_to_file writes; librpcc_rows.so
builds, exports what its header declares and refuses bad arguments; the tools take --stream_decode.  No GPU needed."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import rows_cases as RC  # noqa: E402
import rows_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    import rpcc_amd  # noqa: F401
    from rpcc_amd import _rows_lib
    return _rows_lib


def _saved(tmp_path, pc, w):
    import rpcc_amd  # noqa: F401
    from rpcc_amd.dataset import DatasetTemplate
    f = str(tmp_path / "x.bin")
    with np.errstate(all="ignore"):
        DatasetTemplate.save_point_cloud_to_file(f, pc, intensity=w)
    return open(f, "rb").read()


@pytest.mark.parametrize("with_w", [False, True])
def test_hostile_table_equals_the_saved_file(tmp_path, with_w):
    pc, w = RC.hostile_pc(), RC.hostile_w() if with_w else None
    assert R.kept(pc).tolist() == RC.hostile_kept().tolist() == R.kept_fast(pc).tolist()
    assert True in RC.hostile_kept().tolist() and False in RC.hostile_kept().tolist()
    rows = R.pack(pc, w)
    assert rows.dtype == np.float32 and rows.shape == (int(RC.hostile_kept().sum()), 4)
    assert rows.tobytes() == _saved(tmp_path, pc, w)
    # bits unchanged: -0.0, NaN and the denormal arrive as they were; the fourth column is +0.0 without an intensity
    want = pc.view(np.uint32)[RC.hostile_kept()]
    assert np.array_equal(rows.view(np.uint32)[:, :3], want)
    if with_w:
        assert np.array_equal(rows.view(np.uint32)[:, 3], w.view(np.uint32)[RC.hostile_kept()])
        kept_w = w[RC.hostile_kept()]
        assert np.isnan(kept_w).any() and (np.signbit(kept_w) & (kept_w == 0)).any()      # an intensity of NaN and of -0.0 among the rows
    else:
        assert not rows.view(np.uint32)[:, 3].any()


def test_order_of_the_sum_matters():
    """x + (y + z) keeps (1e8, 1, -1e8)'s rotation that the rule drops: the order is part of the specification."""
    pc = RC.hostile_pc()
    with np.errstate(all="ignore"):
        other = pc[:, 0] + (pc[:, 1] + pc[:, 2]) != 0
    assert (other != R.kept(pc)).any()


@pytest.mark.parametrize("seed,P", [(1, 1), (2, 65), (3, 4099), (4, 28800)])
@pytest.mark.parametrize("with_w", [False, True])
def test_seeded_frames_equal_the_saved_file(tmp_path, seed, P, with_w):
    pc, w, _ = RC.seeded_frame(seed, P)
    if P > 100:
        pc[40: 40 + len(RC.HOSTILE)], w[40: 40 + len(RC.HOSTILE)] = RC.hostile_pc(), RC.hostile_w()
    rows = R.pack(pc, w if with_w else None)
    assert rows.tobytes() == _saved(tmp_path, pc, w if with_w else None)
    if P <= 4099:
        assert np.array_equal(R.kept(pc), R.kept_fast(pc))
    # the package's host rule (the per-frame fallback of BatchDecompressor.decompress_rows) is the same rule
    from rpcc_amd import rows as prows
    assert prows.pack_host(pc, w if with_w else None).tobytes() == rows.tobytes()
    assert prows.pack_host(pc.reshape(1, -1, 3), w if with_w else None).tobytes() == rows.tobytes()


def test_pack_batch_offsets_and_patterns():
    for pattern in RC.PATTERNS:
        pc, w, ri = RC.batch(3, 300, pattern, boundaries=(256,))
        offsets, rows, nonzero = R.pack_batch(pc, w, ri)
        assert offsets[0] == 0 and offsets[-1] == rows.shape[0] and (np.diff(offsets) >= 0).all()
        for b in range(3):
            assert rows[offsets[b]: offsets[b + 1]].tobytes() == R.pack(pc[b], w[b]).tobytes()
            assert nonzero[b] == (ri[b] != 0).sum()
        n = np.diff(offsets)
        if pattern == "all_kept":
            assert n.tolist() == [300] * 3
        if pattern == "none_kept":
            assert n.tolist() == [0] * 3 and pc.any()
        if pattern.startswith("empty_"):
            z = dict(empty_first=0, empty_middle=1, empty_last=2)[pattern]
            assert n[z] == 0 and all(n[b] > 0 for b in range(3) if b != z)


def test_header_symbols_exported(built):
    hdr = open(os.path.join(ROOT, "include", "rpcc_rows.h")).read()
    declared = sorted(set(re.findall(r"\b(rpcc_rows_[a-z0-9_]+)\s*\(", hdr)))
    assert declared == ["rpcc_rows_last_error", "rpcc_rows_pack", "rpcc_rows_version"]
    lib = ctypes.CDLL(built.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    assert built.exported_symbols() == declared
    assert int(re.search(r"#define RPCC_ROWS_ABI_VERSION (\d+)", hdr).group(1)) == built.ABI_VERSION == 1
    assert built.lib().rpcc_rows_version() == built.ABI_VERSION
    for name, val in (("RPCC_ROWS_MAX_BATCH", built.MAX_BATCH), ("RPCC_ROWS_ROUND", built.ROUND), ("RPCC_ROWS_OK", built.OK),
                      ("RPCC_ROWS_E_CAPACITY", built.E_CAPACITY)):
        assert int(re.search(r"#define %s \(?(-?\d+)\)?" % name, hdr).group(1)) == val, name
    assert built.MAX_PIXELS == 1 << 26 and "#define RPCC_ROWS_MAX_PIXELS (1 << 26)" in hdr
    assert built.table_words(5) == 12
    src = open(os.path.join(ROOT, "r-pcc_amd", "csrc_rows", "rows_kernels.hip")).read()
    threads, ppt = (int(re.search(r"#define %s (\d+)" % n, src).group(1)) for n in ("ROWS_THREADS", "ROWS_PPT"))
    assert threads % 64 == 0 and threads * ppt == built.ROUND


def test_argument_errors_do_not_crash(built):
    lib = built.lib()
    raw = ctypes.create_string_buffer(1024 + 64)     # host memory: every call below must refuse before touching it
    base = (ctypes.addressof(raw) + 63) // 64 * 64
    fill = bytes(range(256)) * 4 + b"\0" * 64
    ctypes.memmove(raw, fill, len(fill))
    pc, w, ri, rows, offs, nz = base, base + 128, base + 192, base + 256, base + 512, base + 640
    def call(pc=pc, w=w, ri=ri, B=2, P=4, rows=rows, cap=8, offs=offs, nz=nz, start=None):
        return lib.rpcc_rows_pack(pc, w, ri, B, P, rows, cap, offs, nz, start, None)
    for bad in (dict(pc=None), dict(offs=None), dict(rows=None), dict(B=0), dict(B=-1), dict(B=65536), dict(P=0), dict(P=-3),
                dict(P=(1 << 26) + 1), dict(B=32, P=1 << 26), dict(B=2048, P=1 << 20), dict(cap=-1),
                dict(rows=rows + 8), dict(rows=rows + 4), dict(rows=rows + 1),            # rows must be 16-byte aligned
                dict(offs=offs + 4), dict(pc=pc + 2), dict(w=w + 1), dict(ri=ri + 2), dict(nz=nz + 2), dict(start=offs + 4),
                dict(ri=None)):                                                            # nonzero needs ri_rec
        assert call(**bad) == -1, bad
        assert b"bad argument" in lib.rpcc_rows_last_error(), bad
    assert raw.raw == fill


def test_source_digest_unchanged_by_the_rows_library(built):
    from rpcc_amd import build as b
    before, deps = b.source_digest(), list(b.DEPS)
    b.build_rows(force=True)
    assert b.source_digest() == before and b.DEPS == deps
    assert not any("csrc_rows" in d or d.endswith("rpcc_rows.h") for d in b.DEPS)
    assert os.path.exists(b.ROWS_LIB)
    here = os.path.dirname(b.__file__)
    assert os.path.join(here, "csrc_rows", "rows_kernels.hip") in b.ROWS_DEPS
    assert os.path.join(here, "csrc_tile", "tiles.h") in b.ROWS_DEPS
    assert os.path.join(ROOT, "include", "rpcc_rows.h") in b.ROWS_DEPS


def test_front_end_names_the_missing_gpu(built):
    import torch
    from rpcc_amd import rows
    from rpcc_amd._lib import RpccError
    with pytest.raises(RpccError, match="needs a GPU tensor"):
        rows.pack(torch.zeros((1, 4, 3)))
    with pytest.raises(RpccError, match="needs a GPU tensor"):
        rows.pack(np.zeros((1, 4, 3), np.float32))


def test_parsers_take_stream_decode():
    import rpcc_amd  # noqa: F401
    from rpcc_amd.tools import compress as tc
    p = tc.make_parser(datalist=True)
    off = p.parse_args([])
    assert off.stream_decode is False and off.batch_decode is False
    assert p.parse_args(["--batch_decode"]).stream_decode is False
    on = p.parse_args(["--stream_decode"])
    assert on.stream_decode is True and on.batch_decode is True
    with pytest.raises(SystemExit):
        tc.make_parser().parse_args(["--stream_decode"])      # the single-frame tools have no such flag
