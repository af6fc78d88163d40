"""The .pcd / .ply front ends on the GPU: the points of tests/golden/synth_vlp16.npz written as .pcd in four forms (records of 16 and of 22
bytes, binary_compressed, ASCII) and as .ply give, through tools/compress.py, the container of the same points stored as .bin rows, with and
without --intensity; a datalist of such files through tools/compress_datalist.py (ingest "fields": the files' bytes unpacked on the device)
gives the files of the "rows" ingest byte for byte, also with --subpixel 2 --hidden_points; tools/decompress.py --output x.pcd round-trips.

A frame's identity, which seeds its plane fits, is the CRC of its file name (utils.frame_identity), extension included: the tests pin it to
the name without the extension, so that a .pcd and a .bin of one sweep differ in nothing but their format."""
import os
import zlib

import numpy as np
import pytest
import torch

import pointfile_cases as PC

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GEOM = "VelodyneVLP16"
M = 20
BASE = ["--lidar", GEOM, "--basic_compressor", "bzip2", "--cluster_num", str(M), "--seed", "4"]
FORMS = ("step16.pcd", "step22.pcd", "compressed.pcd", "ascii.pcd", "saved.ply")


def stem_identity(path):
    return zlib.crc32(os.path.basename(str(path).strip()).split(".")[0].encode()) & 0x7FFFFFFF


def write_form(form, path, rows):
    """rows f32 [n,4] -> the file `path` in the named form."""
    from rpcc_amd import pointfile
    from rpcc_amd.dataset import DatasetTemplate
    n = rows.shape[0]
    x, y, z, w = (np.ascontiguousarray(rows[:, c]) for c in range(4))
    if form == "step16.pcd":
        pointfile.write_pcd(path, rows[:, :3], rows[:, 3])
    elif form == "step22.pcd":
        rng = np.random.default_rng(n)
        body, step = PC.packed([("x", "<f4", x), ("y", "<f4", y), ("z", "<f4", z), ("intensity", "<f4", w), ("ring", "<u2", rng.integers(0, 16, n).astype("<u2")),
                                ("time", "<f4", rng.uniform(0, 0.1, n).astype(np.float32))])
        assert step == 22
        open(path, "wb").write(PC.pcd(["x", "y", "z", "intensity", "ring", "time"], (4, 4, 4, 4, 2, 4), "FFFFUF", body, n, count=(1,) * 6, lead="# sweep\n"))
    elif form == "compressed.pcd":
        raw = PC.planes([("x", "<f4", x), ("_", ("u1", 2), None), ("y", "<f4", y), ("z", "<f4", z), ("intensity", "<f4", w)])
        open(path, "wb").write(PC.pcd(["x", "_", "y", "z", "intensity"], (4, 1, 4, 4, 4), "FUFFF", PC.compressed(raw), n, count=(1, 2, 1, 1, 1), data="binary_compressed"))
    elif form == "ascii.pcd":
        text = "".join("%.9g %.9g %.9g %.9g\n" % tuple(r) for r in rows.tolist())
        open(path, "wb").write(PC.pcd(["x", "y", "z", "intensity"], (4,) * 4, "FFFF", text.encode(), n, data="ascii"))
    else:
        assert form == "saved.ply"
        DatasetTemplate.save_point_cloud_to_file(path, rows[:, :3], intensity=rows[:, 3])


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    import __graft_entry__ as ge
    ge.build()
    assert torch.cuda.is_available()
    from rpcc_amd.tools import compress as tc
    from rpcc_amd.tools import compress_datalist as cd
    mp = pytest.MonkeyPatch()
    mp.setattr(tc, "frame_identity", stem_identity)
    mp.setattr(cd, "frame_identity", stem_identity)
    xyz = np.load(os.path.join(HERE, "golden", "synth_vlp16.npz"))["xyz"]
    xyz = xyz[np.sum(xyz, -1) != 0]                 # (what save_point_cloud_to_file keeps)
    rng = np.random.default_rng(25)
    sweeps = []
    for k in range(3):      # the fixture's sweep, and two turned copies of it
        a = 0.3 * k
        rot = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
        pts = (xyz.astype(np.float64) @ rot.T).astype(np.float32)
        sweeps.append(np.concatenate([pts, (rng.integers(0, 256, (pts.shape[0], 1)) / 255).astype(np.float32)], 1))
    d = tmp_path_factory.mktemp("sweeps")
    sweeps[0].tofile(d / "sweep0.bin")
    want = {}
    for flags in ((), ("--intensity",)):
        out = d / ("want%d.rpcc" % len(flags))
        tc.compress(tc.make_parser().parse_args(["--input", str(d / "sweep0.bin"), "--output", str(out)] + BASE + list(flags)))
        want[flags] = out.read_bytes()
    assert want[()] != want[("--intensity",)] and len(want[()]) > 1000
    yield dict(tc=tc, cd=cd, sweeps=sweeps, dir=d, want=want)
    mp.undo()


@pytest.mark.parametrize("form", FORMS)
def test_compress_tool(env, form, tmp_path, capsys):
    from rpcc_amd import pointfile
    tc = env["tc"]
    path = str(tmp_path / ("sweep0." + form.split(".")[1]))
    write_form(form, path, env["sweeps"][0])
    assert np.array_equal(pointfile.read_rows(path).view(np.uint32), env["sweeps"][0].view(np.uint32))
    for flags in ((), ("--intensity",)):
        out = tmp_path / "out.rpcc"
        tc.compress(tc.make_parser().parse_args(["--input", path, "--output", str(out)] + BASE + list(flags)))
        assert out.read_bytes() == env["want"][flags], (form, flags)
    capsys.readouterr()


def test_compress_tool_trailers_and_eval(env, tmp_path, capsys):
    """--intensity --subpixel 2 --hidden_points --eval on a .pcd of 22-byte records: the .bin's container and the .bin's report."""
    tc = env["tc"]
    flags = ["--intensity", "--subpixel", "2", "--hidden_points", "--eval"]
    path = str(tmp_path / "sweep0.pcd")
    write_form("step22.pcd", path, env["sweeps"][0])
    texts = []
    for src, out in ((str(env["dir"] / "sweep0.bin"), tmp_path / "a.rpcc"), (path, tmp_path / "b.rpcc")):
        tc.compress(tc.make_parser().parse_args(["--input", src, "--output", str(out)] + BASE + flags))
        text = capsys.readouterr().out
        texts.append(text[text.index("Reconstruction quality"):])
    assert (tmp_path / "a.rpcc").read_bytes() == (tmp_path / "b.rpcc").read_bytes()
    assert "Intensity Error (max)" in texts[0] and texts[0] == texts[1]


@pytest.mark.parametrize("flags", ((), ("--intensity",), ("--subpixel", "2", "--hidden_points")), ids=("geometry", "intensity", "subpixel-hidden"))
def test_datalist_tool(env, flags, tmp_path):
    """Three files of three forms through ingest "fields" (auto) against the same sweeps as .bin rows through ingest "rows": two batches, the
    last one short."""
    cd = env["cd"]
    from rpcc_amd.tools.compress import make_parser
    names = {"fields": [], "rows": []}
    for k, form in enumerate(("step22.pcd", "compressed.pcd", "saved.ply")):
        for kind in names:
            os.makedirs(tmp_path / kind, exist_ok=True)
        names["fields"].append(str(tmp_path / "fields" / ("sweep%d.%s" % (k, form.split(".")[1]))))
        write_form(form, names["fields"][-1], env["sweeps"][k])
        names["rows"].append(str(tmp_path / "rows" / ("sweep%d.bin" % k)))
        env["sweeps"][k].tofile(names["rows"][-1])
    got = {}
    for kind, lst in names.items():
        (tmp_path / (kind + ".txt")).write_text("".join(n + "\n" for n in lst))
        assert cd.resolve_ingest("auto", lst, intensity="--intensity" in flags, subpixel="--subpixel" in flags, hidden_points="--hidden_points" in flags) == kind
        out = tmp_path / ("out_" + kind)
        cd.compress(make_parser(datalist=True).parse_args(["--datalist", str(tmp_path / (kind + ".txt")), "--output_dir", str(out), "--batch", "2", "--workers", "2"]
                                                          + BASE + list(flags)))
        got[kind] = [open(cd.output_path_for(str(out), n), "rb").read() for n in lst]
    assert len(got["fields"]) == 3 and all(len(b) > 1000 for b in got["rows"]) and got["fields"] == got["rows"]


def test_streaming_ingest_fields(env, tmp_path):
    """Every way a worker places a file in the chunk, in one batch: read in place (records of 16 and 22 bytes, a .ply), LZF-decoded into the
    chunk, parsed from ASCII, and records of a step above RPCC_FIELDS_MAX_STEP through the host reader; slots sized too small, so that they grow."""
    from rpcc_amd import dataset, pipeline, pointfile
    from rpcc_amd.loader import StreamingCompressor
    T = dataset.build_dataset(lidar_type=GEOM).PCTransformer
    mk = lambda: pipeline.BatchCompressor(T, cluster_num=M, accuracy=0.02, basic_compressor="bzip2", seed=4, intensity_scale=255.0)
    rows = env["sweeps"][1][:6000]
    paths = []
    for k, form in enumerate(FORMS):
        paths.append(str(tmp_path / ("f%d.%s" % (k, form.split(".")[1]))))
        write_form(form, paths[-1], rows)
    wide, step = PC.packed([("x", "<f4", rows[:, 0]), ("_", ("u1", 300), None), ("y", "<f4", rows[:, 1]), ("z", "<f4", rows[:, 2]), ("intensity", "<f4", rows[:, 3])])
    assert step == 316 > pointfile.MAX_STEP
    paths.append(str(tmp_path / "wide.pcd"))
    open(paths[-1], "wb").write(PC.pcd(["x", "_", "y", "z", "intensity"], (4, 1, 4, 4, 4), "FUFFF", wide, rows.shape[0], count=(1, 300, 1, 1, 1)))
    fids = list(range(40, 40 + len(paths)))
    got = {}
    sc = StreamingCompressor(mk(), batch=4, depth=2, workers=2, ingest="fields", points_per_frame=1000)
    assert sc.run([(paths[:4], fids[:4]), (paths[4:], fids[4:])], sink=lambda k, blobs: got.update({k: blobs})) == len(paths)
    assert sc.grown >= 1 and all(s.xyz_pin is None and s.xyz_dev.shape[1] == 4 for s in sc.slots)
    want = mk().compress([rows] * len(paths), frame_ids=fids)
    assert got[0] + got[1] == want
    bad = tmp_path / "bad.pcd"
    bad.write_bytes([c for c in PC.CASES if c[0] == "refuse_short_body"][0][2])
    with pytest.raises(ValueError, match="the body holds"):
        sc.run([([str(bad)], [0])])
    with pytest.raises(ValueError, match="takes the paths"):
        sc.run([([rows], [0])])


def test_decompress_to_pcd_round_trips(env, tmp_path, capsys):
    from rpcc_amd import pointfile
    from rpcc_amd.tools import decompress as td
    tc = env["tc"]
    src = tmp_path / "a.rpcc"
    src.write_bytes(env["want"][("--intensity",)])
    for out in ("x.pcd", "x.bin"):
        td.decompress(td.make_parser().parse_args(["--input", str(src), "--output", str(tmp_path / out), "--intensity"] + BASE))
    back = pointfile.read_rows(str(tmp_path / "x.pcd"))
    assert back.shape[0] > 10000 and np.array_equal(back.view(np.uint32), np.fromfile(tmp_path / "x.bin", np.float32).reshape(-1, 4).view(np.uint32))
    assert (tmp_path / "x.pcd").read_bytes().startswith(pointfile.pcd_header(back.shape[0], True))
    # the decoded file goes in again, and --eval reads the original from a .pcd as it does from the .bin
    for name in ("x.pcd", "x.bin"):
        tc.compress(tc.make_parser().parse_args(["--input", str(tmp_path / name), "--output", str(tmp_path / (name + ".rpcc")), "--intensity"] + BASE))
    assert (tmp_path / "x.pcd.rpcc").read_bytes() == (tmp_path / "x.bin.rpcc").read_bytes()
    capsys.readouterr()
    texts = []
    orig_pcd = str(tmp_path / "sweep0.pcd")
    write_form("step22.pcd", orig_pcd, env["sweeps"][0])
    for orig in (orig_pcd, str(env["dir"] / "sweep0.bin")):
        td.decompress(td.make_parser().parse_args(["--input", str(src), "--output", str(tmp_path / "y.pcd"), "--intensity", "--eval",
                                                   "--original_point_cloud", orig] + BASE))
        text = capsys.readouterr().out
        texts.append(text[text.index("    BPP: "):])
    assert "Intensity Error (max)" in texts[0] and texts[0] == texts[1]
