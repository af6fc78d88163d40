"""The per-beam table entries without a GPU: symbols and interface version, header and bindings in step, the host-side index builder
against numpy (and as a stand-alone program under the address / undefined-behaviour sanitizers), scratch and workspace sizes, argument
errors raised before the device is touched, CSV parsing and the three refusals, and PCTransformer(cfg, csv) constructing."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import beam_table_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CFG = os.path.join(ROOT, "r-pcc_amd", "lidar_cfg")
YAML, CSV = os.path.join(CFG, "Velodyne_HDL_64E.yaml"), os.path.join(CFG, "Velodyne_HDL_64E_beams.csv")
NEW = ("rpcc_beam_index_bytes", "rpcc_beam_index_build", "rpcc_project_beams_scratch_bytes", "rpcc_project_beams", "rpcc_project_beams_check",
       "rpcc_compress_batch_beams_workspace_bytes", "rpcc_compress_batch_beams")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    import rpcc_amd  # noqa: F401
    from rpcc_amd import _lib
    return _lib


def test_symbols_version_header_and_bindings(built):
    lib = ctypes.CDLL(built.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "rpcc_hip.h")).read()
    integ = open(os.path.join(ROOT, "integration", "rpcc_hip_binding.py")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in built.exported_symbols()
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    for name in ("rpcc_beam_index_bytes", "rpcc_beam_index_build", "rpcc_project_beams_scratch_bytes", "rpcc_project_beams"):
        assert name in integ, name
    assert built.lib().rpcc_version() == built.ABI_VERSION == 105
    assert "#define RPCC_ABI_VERSION 105" in hdr and "RPCC_ABI_VERSION = 105" in integ
    assert int(re.search(r"#define RPCC_BEAM_MAX_H (\d+)", hdr).group(1)) == built.BEAM_MAX_H == R.BEAM_MAX_H == 128


def test_index_builder_equals_numpy(built):
    from rpcc_amd import ops
    rng = np.random.default_rng(5)
    tables = [R.read_csv(CSV), np.array([0.3]), np.array([0.1, -0.2]), np.radians([-10.0, -2.0, -10.0, -2.0, 1.0]), np.zeros(7),
              np.array([0.0, -0.0, 0.0]), rng.permutation(np.linspace(-0.4, 0.1, 128)),
              np.array([0.1, np.nextafter(0.1, 1.0), np.nextafter(np.float32(0.1), np.float32(1)).astype(np.float64)])]
    for va in tables:
        H = len(va)
        assert built.lib().rpcc_beam_index_bytes(H) == 24 * H
        got = ops.beam_index_host(va)
        assert got.dtype == np.uint8 and got.tobytes() == R.index_bytes(va), H
        a, s, mid, row = R.beam_index(va)
        assert np.all(np.diff(s) >= 0) and np.array_equal(va[row], s)
        assert all(row[k] == np.flatnonzero(va == s[k])[0] for k in range(H))                   # equal entries: the lowest row
    assert built.lib().rpcc_beam_index_bytes(0) == 0 and built.lib().rpcc_beam_index_bytes(129) == 0
    out = np.zeros(24 * 3, np.uint8)
    for bad in (np.array([0.1, np.nan, 0.2]), np.array([0.1, np.inf, 0.2])):
        assert built.lib().rpcc_beam_index_build(bad.ctypes.data_as(ctypes.c_void_p), 3, out.ctypes.data_as(ctypes.c_void_p)) == -1
        assert b"rpcc_beam_index_build" in built.lib().rpcc_last_error() and not out.any()


@pytest.mark.parametrize("sanitize", (False, True))
def test_index_builder_as_a_host_program(tmp_path, sanitize):
    """csrc/beam_index.h built into tests/beam_index_host_main.cpp: H = 1 .. 128, sorted / descending / shuffled / constant / duplicated tables into
    heap blocks of the exact size; every index equals numpy's.  sanitize: the same under -fsanitize=address,undefined."""
    exe = str(tmp_path / "beam_index_host")
    cmd = [os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-I", os.path.join(ROOT, "r-pcc_amd", "csrc"),
           os.path.join(HERE, "beam_index_host_main.cpp"), "-o", exe]
    if sanitize:
        cmd[1:1] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]   # (runtimes inside the program)
    subprocess.check_call(cmd)
    r = subprocess.run([exe, str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0 and "640 tables OK" in r.stdout, (r.stdout, r.stderr)
    got = open(tmp_path / "out.bin", "rb").read()
    pos = n = 0
    while pos < len(got):
        H, = struct.unpack_from("<q", got, pos)
        idx = got[pos + 8: pos + 8 + 24 * H]
        assert idx == R.index_bytes(np.frombuffer(idx[: 8 * H], dtype=np.float64)), (n, H)
        pos += 8 + 24 * H
        n += 1
    assert n == 640 and pos == len(got)


def test_sizes(built):
    lib = built.lib()
    for total, B, P in ((0, 1, 16), (122320, 1, 128000), (3 * 122320 + 7, 3, 128000), (5, 2, 5 * 8)):
        n = lib.rpcc_project_beams_scratch_bytes(total, B, P)
        assert n % 256 == 0 and 4 * B * P + 4 * total <= n <= 4 * B * P + 4 * total + 768
        assert n <= lib.rpcc_project_scratch_bytes(total, B, P)        # fits the fused batch's projection area
    assert lib.rpcc_project_beams_scratch_bytes(10, 0, 16) == 0 and lib.rpcc_project_beams_scratch_bytes(-1, 1, 16) == 0
    P = 64 * 2000
    for M in (1, 100, 254):
        assert lib.rpcc_compress_batch_beams_workspace_bytes(4, P, M, 500000, 0) == lib.rpcc_workspace_bytes(4, P, M, 500000)
        assert lib.rpcc_compress_batch_beams_workspace_bytes(4, P, M, 500000, 1) == lib.rpcc_workspace_bytes_general(4, P, M, 500000)
    for M in (255, 300, 1022):
        assert lib.rpcc_compress_batch_beams_workspace_bytes(4, P, M, 500000, 0) == lib.rpcc_wide_workspace_bytes(4, P, M, 500000)
    for B, P_, M in ((0, P, 100), (4, 0, 100), (4, P, 0), (4, P, 1023), (4, P, 65533)):
        assert lib.rpcc_compress_batch_beams_workspace_bytes(B, P_, M, 0, 1) == 0


def test_argument_errors_before_the_device(built):
    """Every pointer is a host dummy that must never reach a kernel: the calls return RPCC_ERR_ARG first."""
    lib = built.lib()
    dummy = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(dummy) + 255) & ~255
    geom = built.Geom(64, 2000, 6.2831855, 0.0, 0.0)

    def proj(points=p, stride=12, offs=p, total=100, B=1, g=geom, beams=p, ri=p, scratch=p, nbytes=1 << 30):
        return lib.rpcc_project_beams(points, stride, offs, total, B, g, beams, ri, scratch, nbytes, None)

    for kw in (dict(points=None), dict(offs=None), dict(beams=None), dict(ri=None), dict(scratch=None), dict(stride=8), dict(stride=16, points=p + 4),
               dict(total=-1), dict(total=1 << 31), dict(B=0), dict(B=65536), dict(beams=p + 4), dict(nbytes=1000),
               dict(g=built.Geom(129, 2000, 6.28, 0.0, 0.0)), dict(g=built.Geom(0, 2000, 6.28, 0.0, 0.0)), dict(g=built.Geom(64, 0, 6.28, 0.0, 0.0)),
               dict(g=built.Geom(64, 2000, 0.0, 0.0, 0.0)), dict(g=built.Geom(64, 2000, float("nan"), 0.0, 0.0)),
               dict(g=built.Geom(128, 1 << 24, 6.28, 0.0, 0.0)), dict(g=built.Geom(2, 1 << 30, 6.28, 0.0, 0.0))):      # H * W does not fit an int
        assert proj(**kw) == -1 and b"bad argument" in lib.rpcc_last_error(), kw
    assert lib.rpcc_project_beams_check(None, 10, geom, p, p, None) == -1
    assert lib.rpcc_project_beams_check(p, 0, geom, p, p, None) == -1
    io = built.BatchIO(p, p, 1000, p, p, -1, None, p, p, p, p, p, p, p, p, p, 0, None, 0, 0.0, 0, None, None, None, 12)

    def fused(io=io, B=2, g=geom, beams=p, M=100, ws=p):
        return lib.rpcc_compress_batch_beams(ctypes.byref(io) if io is not None else None, B, g, beams, M, 0.1, 0.04, ws, None)

    for kw in (dict(io=None), dict(beams=None), dict(ws=None), dict(M=0), dict(M=1023), dict(M=65533), dict(B=0),
               dict(g=built.Geom(129, 2000, 6.28, 0.0, 0.0)), dict(g=built.Geom(64, 2000, -1.0, 0.0, 0.0)),
               dict(g=built.Geom(128, 1 << 24, 6.28, 0.0, 0.0))):
        assert fused(**kw) == -1 and b"bad argument" in lib.rpcc_last_error(), kw
    bad = built.BatchIO(p, p, 1000, p, p, -1, None, p, p, p, p, p, p, p, p, p, 16, None, 0, 0.0, 0, None, None, None, 12)
    assert fused(io=bad) == -1 and b"flags" in lib.rpcc_last_error()


def _csv(path, deg, header="channel,vertical_angle"):
    with open(path, "w") as f:
        f.write(header + "\n" + "".join("%d,%r\n" % (i, float(v)) for i, v in enumerate(deg)))
    return str(path)


def test_transformer_takes_a_csv(built, tmp_path):
    """PCTransformer(lidar_cfg, channel_distribute_csv) constructs (no device is touched before a point cloud arrives) and refuses what the
    reference would mis-handle."""
    from rpcc_amd import ops
    from rpcc_amd.transformer import PCTransformer, read_channel_csv
    from rpcc_amd.dataset import DatasetTemplate
    T = PCTransformer(YAML, CSV)
    assert T.even_dist is False and T.H == 64 and T.W == 2000
    assert T.vertical_angle.dtype == np.float64 and np.array_equal(T.vertical_angle, R.read_csv(CSV))
    assert np.array_equal(T.transform_map.view(np.uint32), R.transform_map(T.vertical_angle, T.horizontal_FOV, 64, 2000).view(np.uint32))
    E = PCTransformer(YAML)
    assert E.even_dist is True and E.beams_dev is None and not np.array_equal(E.transform_map, T.transform_map)
    assert DatasetTemplate(None, YAML, CSV).PCTransformer.even_dist is False
    # line h of the file is row h, whatever `channel` says; unsorted tables are taken as they are
    deg = list(np.linspace(2.0, -24.0, 64))
    p = _csv(tmp_path / "desc.csv", deg)
    assert np.array_equal(read_channel_csv(p), np.radians(np.array(deg)))
    assert np.array_equal(PCTransformer(YAML, p).vertical_angle, np.radians(np.array(deg)))
    with pytest.raises(ValueError, match="63 vertical angles for RANGE_IMAGE_HEIGHT = 64"):
        PCTransformer(YAML, _csv(tmp_path / "short.csv", deg[:63]))
    with pytest.raises(ValueError, match="entry 5 is not finite"):
        PCTransformer(YAML, _csv(tmp_path / "nan.csv", deg[:5] + [float("nan")] + deg[6:]))
    with pytest.raises(ValueError, match="entry 0 is not finite"):
        PCTransformer(YAML, _csv(tmp_path / "inf.csv", [float("inf")] + deg[1:]))
    tall = dict(HORIZONTAL_FOV=360, VERTICAL_ANGLE_MAX=2.0, VERTICAL_ANGLE_MIN=-24.9, RANGE_IMAGE_HEIGHT=129, RANGE_IMAGE_WIDTH=64)
    with pytest.raises(ValueError, match="129 rows.*128"):
        PCTransformer(tall, _csv(tmp_path / "tall.csv", list(np.linspace(-20, 2, 129))))
    with pytest.raises(ValueError):
        ops.beam_table([0.1, 0.2], H=3)


def test_front_ends_that_have_no_table_form(built):
    from rpcc_amd.pipeline import BatchCompressor, MixedBatchCompressor
    from rpcc_amd.transformer import PCTransformer
    T, E = PCTransformer(YAML, CSV, device="cpu"), PCTransformer(YAML, device="cpu")
    with pytest.raises(NotImplementedError, match="per-beam elevation table.*cluster_num <= 1022"):
        BatchCompressor(T, cluster_num=2000)
    BatchCompressor(T, cluster_num=1022)
    with pytest.raises(NotImplementedError, match=r"\['b'\].*per-beam elevation table"):
        MixedBatchCompressor({"a": E, "b": T})
    from rpcc_amd.tools.compress import make_parser
    for datalist in (False, True):
        a = make_parser(datalist=datalist).parse_args(["--channel_distribute_csv", CSV])
        assert a.channel_distribute_csv == CSV
        assert make_parser(datalist=datalist).parse_args([]).channel_distribute_csv is None
