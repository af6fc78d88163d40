"""librpcc_fields.so (include/rpcc_fields.h) builds, exports what its header declares and refuses bad arguments before the device is
touched; csrc/, build.DEPS and source_digest() do not change with it.  The front ends without a GPU: resolve_ingest on .pcd / .ply names,
load_data / load_rows on files, the unchanged refusals of --input_format.  No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    import rpcc_amd  # noqa: F401
    from rpcc_amd import _fields_lib
    return _fields_lib


def test_header_symbols_exported(built):
    hdr = open(os.path.join(ROOT, "include", "rpcc_fields.h")).read()
    declared = sorted(set(re.findall(r"\b(rpcc_[a-z0-9_]+)\s*\(", hdr)))
    assert declared == ["rpcc_fields_last_error", "rpcc_fields_unpack", "rpcc_fields_version"]
    lib = ctypes.CDLL(built.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    assert built.exported_symbols() == declared
    assert int(re.search(r"#define RPCC_FIELDS_ABI_VERSION (\d+)", hdr).group(1)) == built.ABI_VERSION == 1
    from rpcc_amd import pointfile
    import fields_caps as FC
    import fields_ref as FR
    for name, val in (("RPCC_FIELDS_DESC_WORDS", built.DESC_WORDS), ("RPCC_FIELDS_MAX_STEP", built.MAX_STEP), ("RPCC_FIELDS_MAX_TOTAL", built.MAX_TOTAL),
                      ("RPCC_FIELDS_MAX_BATCH", built.MAX_BATCH), ("RPCC_FIELDS_OK", built.OK), ("RPCC_FIELDS_E_LAYOUT", built.E_LAYOUT)):
        assert int(re.search(r"#define %s \(?(-?\d+)\)?" % name, hdr).group(1)) == val, name
    assert pointfile.DESC_WORDS == built.DESC_WORDS == FR.DESC_WORDS == 16 and pointfile.MAX_STEP == built.MAX_STEP == FC.MAX_STEP == 256
    rule = open(os.path.join(ROOT, "r-pcc_amd", "csrc_fields", "fields_rule.h")).read()
    for k, name in enumerate(pointfile.TYPE_NAMES):      # one numbering in the header, the rule, the module and the tests
        assert int(re.search(r"#define RPCC_FIELDS_T_%s (\d+)" % name, hdr).group(1)) == k == getattr(pointfile, name) == getattr(FR, name)
        assert int(re.search(r"#define FIELDS_T_%s (\d+)" % name, rule).group(1)) == k
    assert FR.SIZE == pointfile.TYPE_SIZE
    assert FC.FLD_THREADS % 64 == 0 and FC.FLD_GRID_CAP >= 1 and FC.tile_rows(FC.MAX_STEP) >= 1 and FC.tile_rows(1) == FC.TILE_MAX_ROWS and FC.TILE_MAX_ROWS % FC.FLD_THREADS == 0


def test_version(built):
    assert built.lib().rpcc_fields_version() == built.ABI_VERSION


def test_argument_errors_do_not_crash(built):
    lib = built.lib()
    raw = ctypes.create_string_buffer(1024 + 64)     # host memory: every call below must refuse before touching it
    base = (ctypes.addressof(raw) + 63) // 64 * 64
    fill = bytes(range(256)) * 4 + b"\0" * 64
    ctypes.memmove(raw, fill, len(fill))
    chunk, desc, offs, rows, status = base, base + 256, base + 512, base + 640, base + 896      # 64 chunk bytes, 2 descriptors, 3 offsets, 8 rows, 2 words
    call = lambda bytes_=chunk, nbytes=64, d=desc, B=2, ro=offs, total=8, out=rows, st=status: lib.rpcc_fields_unpack(bytes_, nbytes, d, B, ro, total, out, st, None)
    for bad in (dict(B=-1), dict(B=2 ** 20 + 1), dict(total=-1), dict(total=2 ** 31), dict(nbytes=-1), dict(d=None), dict(ro=None), dict(st=None),
                dict(bytes_=None), dict(out=None), dict(bytes_=chunk + 8), dict(bytes_=chunk + 1), dict(out=rows + 8), dict(d=desc + 4), dict(ro=offs + 2),
                dict(st=status + 2), dict(bytes_=rows, nbytes=16), dict(bytes_=rows + 112, nbytes=64), dict(out=chunk + 48),      # rows over the chunk
                dict(B=0, total=8), dict(B=0, bytes_=chunk + 1, total=0)):
        assert call(**bad) == -1, bad
        assert b"bad argument" in lib.rpcc_fields_last_error(), bad
    assert raw.raw == fill
    assert lib.rpcc_fields_unpack(None, 0, None, 0, None, 0, None, None, None) == 0      # no frames: nothing is launched
    assert call(B=0, total=0) == 0 and raw.raw == fill


def test_source_digest_unchanged_by_the_fields_library(built):
    from rpcc_amd import build as b
    before, deps = b.source_digest(), list(b.DEPS)
    b.build_fields(force=True)
    b.build_host(force=True)
    assert b.source_digest() == before and b.DEPS == deps
    assert not any("csrc_fields" in d or d.endswith("rpcc_fields.h") for d in b.DEPS)
    assert os.path.exists(b.FIELDS_LIB)
    here = os.path.dirname(b.__file__)
    assert os.path.join(here, "csrc_fields", "fields_rule.h") in b.FIELDS_DEPS
    assert os.path.join(here, "csrc_tile", "tiles.h") in b.FIELDS_DEPS      # the shared error state
    assert os.path.join(ROOT, "include", "rpcc_fields.h") in b.FIELDS_DEPS


def test_front_ends_name_the_missing_gpu(built):
    import torch
    from rpcc_amd import pointfile
    from rpcc_amd._lib import RpccError
    d = [pointfile.stored_layout(2).desc(0)]
    with pytest.raises(RpccError, match="needs a GPU tensor"):
        pointfile.unpack(torch.zeros(32, dtype=torch.uint8), d)
    with pytest.raises(RpccError, match="needs a GPU tensor"):
        pointfile.unpack(np.zeros(32, np.uint8), d)


def test_resolve_ingest(built):
    from rpcc_amd.tools.compress_datalist import resolve_ingest
    assert resolve_ingest("auto", ["a/1.pcd", "a/2.pcd"]) == "fields"
    assert resolve_ingest("auto", ["a/1.ply"]) == "fields"
    assert resolve_ingest("auto", ["a/1.pcd", "a/2.ply"]) == "fields"
    for kw in (dict(intensity=True), dict(subpixel=True), dict(hidden_points=True), dict(intensity=True, subpixel=True, hidden_points=True)):
        assert resolve_ingest("auto", ["a/1.pcd", "a/2.ply"], **kw) == "fields"      # 16-byte rows on the device: the trailers go with it
    assert resolve_ingest("auto", ["a/1.pcd", "a/2.bin"]) == "xyz"                     # mixed: the host path through load_data
    assert resolve_ingest("auto", ["a/1.pcd", "a/2.txt"]) == "xyz"
    assert resolve_ingest("xyz", ["a/1.pcd"]) == "xyz"
    assert resolve_ingest("auto", []) == "xyz"
    assert resolve_ingest("auto", ["a/1.bin"]) == "rows" and resolve_ingest("auto", ["a/1.bin"], point_format="nclt") == "nclt"
    # every existing message for other names, word for word
    with pytest.raises(SystemExit) as e:
        resolve_ingest("auto", ["a/1.pcd", "a/2.bin"], intensity=True)
    assert str(e.value) == "--intensity needs a datalist of .bin files (float32 rows x, y, z, intensity)"
    with pytest.raises(SystemExit) as e:
        resolve_ingest("rows", ["a/1.pcd"])
    assert str(e.value) == "--ingest rows needs a datalist of .bin files (float32 rows x, y, z, intensity)"
    with pytest.raises(SystemExit) as e:
        resolve_ingest("auto", ["a/1.txt"], subpixel=True)
    assert str(e.value).startswith("--subpixel on a datalist needs .bin files: its kernels read 16-byte rows")


def test_load_data_and_load_rows(built, tmp_path):
    import pointfile_cases as PC
    from rpcc_amd.dataset import DatasetTemplate as D, build_dataset
    for name in ("velodyne_step22_odd_header", "xyz_f32_step12", "ascii_pcd", "binary_compressed_planes", "ply_short_names_face_after_vertex", "ascii_ply"):
        _, fmt, data, want = [c for c in PC.CASES if c[0] == name][0]
        path = str(tmp_path / (name + "." + fmt))
        open(path, "wb").write(data)
        pts, rows = D.load_data(path), D.load_rows(path)
        assert pts.dtype == np.float32 and pts.shape == (want.shape[0], 3) and rows.shape == want.shape
        assert np.array_equal(rows.view(np.uint32), want.view(np.uint32)) and np.array_equal(pts.view(np.uint32), want[:, :3].view(np.uint32))
    assert not rows[:, 3].any() or name != "xyz_f32_step12"
    with pytest.raises(ValueError, match="no field z"):
        bad = [c for c in PC.CASES if c[0] == "refuse_missing_z"][0]
        open(tmp_path / "bad.pcd", "wb").write(bad[2])
        D.load_data(str(tmp_path / "bad.pcd"))
    with pytest.raises(ValueError, match="intensity is read from"):      # unchanged: three columns of an .npz say nothing about intensity
        D.load_rows(str(tmp_path / "x.npz"))
    with pytest.raises(AssertionError, match="File type not correct"):
        D.load_data(str(tmp_path / "x.las"))


def test_input_format_keeps_its_refusals(built):
    from rpcc_amd import records
    from rpcc_amd.tools.compress import make_parser
    for p in (make_parser(), make_parser(datalist=True)):
        for fmt in ("pcd", "ply", "fields"):
            with pytest.raises(SystemExit):
                p.parse_args(["--input_format", fmt])
    for fmt in ("pcd", "ply", "fields"):
        with pytest.raises(ValueError, match="point_format"):
            records.check_point_format(fmt)
    assert records.POINT_FORMATS == (None, "nclt")
