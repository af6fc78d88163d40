"""-m gpu: the .bin row packer (librpcc_rows.so, rows.py) against tests/rows_ref.py by bits; BatchDecompressor.decompress_rows against the
per-frame path (decode_frame, then save_point_cloud_to_file) byte for byte; loader.StreamingDecompressor and --stream_decode against the
files --batch_decode writes.

1. the kernels at B in {1, 3} and P in {1, 65, one round, two rounds and a tail}: every frame pattern of tests/rows_cases.py, with and
   without intensity and ri_rec, rows of exactly `total` rows between guards from a 0xFF and a 0x00 fill, a capacity one row short, and two
   calls chained through `base`;  2. decompress_rows over back-ends, frameworks, label widths, DBSCAN and intensity streams;  3. a chunk
   with a host fallback and a refusal;  4. the streaming front end and the tool."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import buffer_arena as BA  # noqa: E402
import rows_cases as RC  # noqa: E402
import rows_ref as R  # noqa: E402

ACC = 0.02
DELTA = (0, 0.02, 0.04, 0.06)
LACC = np.array([2 * ACC] * 4) + np.array(DELTA)
LIDARS = {"VelodyneVLP16": "synth_vlp16", "Velodyne32E": "synth_32E"}


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    import rpcc_amd  # noqa: F401
    from rpcc_amd import _lib, _rows_lib, compress_utils, dataset, loader, pipeline, rows, synth
    from rpcc_amd.tools.decompress import decode_frame
    from oracle import oracle as orc
    return dict(torch=torch, lib=_lib, rl=_rows_lib, rows=rows, cu=compress_utils, ds=dataset, loader=loader, pl=pipeline, synth=synth,
                dec=decode_frame, orc=orc, dev=torch.device("cuda:0"), cache={})


# ------------------------------------------------------------------------------------------------
# 1. the kernels
# ------------------------------------------------------------------------------------------------
def _round(env):
    return env["rl"].ROUND


def _dev(env, a):
    return None if a is None else env["torch"].from_numpy(np.ascontiguousarray(a)).to(env["dev"])


def _bits(t):
    return t.detach().cpu().contiguous().numpy().reshape(-1).view(np.uint8)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("Pk", ["1", "65", "round", "2 rounds + 3"])
def test_kernel_equals_reference_by_bits(env, B, Pk):
    torch, rows_mod, rl = env["torch"], env["rows"], env["rl"]
    RND = _round(env)
    assert RND % 256 == 0
    P = {"1": 1, "65": 65, "round": RND, "2 rounds + 3": 2 * RND + 3}[Pk]
    bounds = (256, RND, 2 * RND)          # a wavefront's last pixel | first of the next; a round's last | first of the next
    words = rl.table_words(B)
    table = BA.Arena(8 * words, env["dev"], back=1 << 12)
    nz = BA.Arena(4 * B, env["dev"], back=1 << 12)
    seen_totals = set()
    for pattern in RC.PATTERNS:
        pc, w, ri = RC.batch(B, P, pattern, boundaries=bounds, seed=3)
        combos = [(True, True), (False, False)] + ([(True, False), (False, True)] if pattern == "mixed" else [])
        for with_w, with_ri in combos:
            offsets, want, nonzero = R.pack_batch(pc, w if with_w else None, ri if with_ri else None)
            total = int(offsets[-1])
            seen_totals.add(total)
            d_pc, d_w, d_ri = _dev(env, pc), _dev(env, w if with_w else None), _dev(env, ri if with_ri else None)
            arena = BA.Arena(max(16 * total, 16), env["dev"], back=1 << 14)
            out = arena.view[: 16 * total].view(torch.float32).view(total, 4)
            assert total == 0 or out.data_ptr() % 16 == 0
            for fill in ("ones", "zero"):                      # the same buffers twice, whatever they held
                arena.fill(fill), table.fill(fill), nz.fill(fill)
                t, r, n = rows_mod.pack(d_pc, d_w, d_ri, rows=out, table=table.view.view(torch.int64), nonzero=nz.view.view(torch.int32))
                torch.cuda.synchronize()
                tag = (B, P, pattern, with_w, with_ri, fill)
                assert arena.check_guards() is None and table.check_guards() is None and nz.check_guards() is None, tag
                tab = t.cpu().numpy()
                assert tab[: B + 1].tolist() == offsets.tolist() and tab[B + 1] == rl.OK, tag
                assert tab[B + 2:].tolist() == np.diff(offsets).tolist(), tag
                bad = np.flatnonzero(_bits(r) != want.reshape(-1).view(np.uint8))
                assert bad.size == 0, (tag, bad.size, bad[:6])
                if total == 0:
                    assert (arena.view == (0xFF if fill == "ones" else 0)).all(), tag      # nothing kept: nothing written
                if with_ri:
                    assert n.cpu().numpy().tolist() == nonzero.tolist(), tag
                else:
                    assert n is None and _bits(nz.view).tolist() == ([0xFF] * (4 * B) if fill == "ones" else [0] * (4 * B)), tag
            if total and with_w == with_ri:
                # a capacity one row short: rows untouched, the true offsets, the status set
                short = BA.Arena(max(16 * (total - 1), 16), env["dev"], back=1 << 14).fill("ones")
                small = short.view[: 16 * (total - 1)].view(torch.float32).view(total - 1, 4)
                t, _, _ = rows_mod.pack(d_pc, d_w, d_ri, rows=small)
                torch.cuda.synchronize()
                tab = t.cpu().numpy()
                assert tab[: B + 1].tolist() == offsets.tolist() and tab[B + 1] == rl.E_CAPACITY, (B, P, pattern)
                assert short.check_guards() is None and bool((short.view == 0xFF).all()), (B, P, pattern)
    assert 0 in seen_totals and B * P in seen_totals        # none kept and all kept were among them
    # the default buffers: B * P rows always suffice
    pc, w, ri = RC.batch(B, P, "mixed", boundaries=bounds, seed=4)
    offsets, want, nonzero = R.pack_batch(pc, w, ri)
    t, r, n = rows_mod.pack(_dev(env, pc).view(B, 1, P, 3), _dev(env, w).view(B, 1, P), _dev(env, ri).view(B, 1, P))
    assert r.shape == (B * P, 4) and t.cpu().numpy()[: B + 2].tolist() == offsets.tolist() + [rl.OK]
    assert np.array_equal(_bits(r[: int(offsets[-1])]), want.reshape(-1).view(np.uint8)) and n.cpu().numpy().tolist() == nonzero.tolist()


def test_calls_chained_through_base(env):
    """Two calls into one rows buffer, the second starting where the first ended without the host knowing where: the batch's rows, and a
    capacity that the two together exceed is reported by the second call alone."""
    torch, rows_mod, rl = env["torch"], env["rows"], env["rl"]
    P = _round(env) + 77
    pc, w, ri = RC.batch(5, P, "empty_middle", boundaries=(256, _round(env)), seed=9)
    offsets, want, nonzero = R.pack_batch(pc, w, ri)
    total = int(offsets[-1])
    for cap, status in ((total, rl.OK), (total - 1, rl.E_CAPACITY)):
        arena = BA.Arena(16 * cap, env["dev"], back=1 << 14).fill("ones")
        out = arena.view.view(torch.float32).view(cap, 4)
        t1, _, n1 = rows_mod.pack(_dev(env, pc[:2]), _dev(env, w[:2]), _dev(env, ri[:2]), rows=out)
        t2, _, n2 = rows_mod.pack(_dev(env, pc[2:]), _dev(env, w[2:]), _dev(env, ri[2:]), rows=out, base=t1[2:3])
        torch.cuda.synchronize()
        a, b = t1.cpu().numpy(), t2.cpu().numpy()
        assert a[:3].tolist() == offsets[:3].tolist() and a[3] == rl.OK
        assert b[:4].tolist() == offsets[2:].tolist() and b[4] == status
        assert n1.cpu().numpy().tolist() + n2.cpu().numpy().tolist() == nonzero.tolist()
        assert arena.check_guards() is None
        first = int(offsets[2])
        assert np.array_equal(_bits(out[:first]), want[:first].reshape(-1).view(np.uint8))
        if status == rl.OK:
            assert np.array_equal(_bits(out), want.reshape(-1).view(np.uint8))
        else:
            assert bool((arena.view[16 * first:] == 0xFF).all())


# ------------------------------------------------------------------------------------------------
# 2. decompress_rows against the per-frame path
# ------------------------------------------------------------------------------------------------
def _T(env, lidar):
    key = ("T", lidar)
    if key not in env["cache"]:
        env["cache"][key] = env["ds"].build_dataset(lidar_type=lidar).PCTransformer
    return env["cache"][key]


def _frames(env, lidar, n=2):
    """The committed sweep of the geometry and n - 1 synthetic ones beside it."""
    gd = env["orc"].GEOMS[lidar]
    xyz = np.load(os.path.join(HERE, "golden", LIDARS[lidar] + ".npz"))["xyz"]
    return [xyz] + [env["synth"].make_frame(7300 + i, gd["H"], gd["W"], vmax_deg=gd["vmax_deg"], vmin_deg=gd["vmin_deg"]).numpy() for i in range(n - 1)]


def _containers(env, lidar, M, uniform, method, n=2):
    key = (lidar, M, uniform, method, n)
    if key not in env["cache"]:
        cfg = dict(env["orc"].DEFAULT_CFG, cluster_num=M, accuracy=ACC)
        bc = env["pl"].BatchCompressor(_T(env, lidar), cluster_num=M, accuracy=ACC, uniform=uniform, compressor_cfg=cfg, basic_compressor=method, seed=3)
        env["cache"][key] = bc.compress(_frames(env, lidar, n))
    return env["cache"][key]


def _per_frame_file(env, tmp_path, blob, T, M, accuracy, lacc, uniform, method, intensity=False):
    """decode_frame, then save_point_cloud_to_file: the .bin bytes of the per-frame tool, and its point count."""
    cu = env["cu"]
    rec, pc, _, *w = env["dec"](cu.unpack_bitstream(blob, uniform, intensity=intensity), cu.BasicCompressor(method_name=method), T, M, accuracy, lacc,
                                uniform, intensity=intensity)
    f = str(tmp_path / "per_frame.bin")
    env["ds"].DatasetTemplate.save_point_cloud_to_file(f, pc.reshape(-1, 3), intensity=w[0].reshape(-1) if w else None)
    return open(f, "rb").read(), int((rec != 0).sum())


def _check(env, tmp_path, bd, blobs, T, M, accuracy, lacc, uniform, method, intensity=False, tag=None):
    """decompress_rows against the per-frame files; -> [(rows, the per-frame path's point count)].  The device form's nonzero is that count
    for every frame the device decoded."""
    got = bd.decompress_rows(blobs)
    status, _, _, nonzero = bd.decompress_rows_device(blobs)
    status, nonzero = status.cpu().tolist(), nonzero.cpu().tolist()
    assert len(got) == len(blobs)
    out = []
    for i, (blob, rows) in enumerate(zip(blobs, got)):
        want, points = _per_frame_file(env, tmp_path, blob, T, M, accuracy, lacc, uniform, method, intensity)
        assert rows.dtype == np.float32 and rows.ndim == 2 and rows.shape[1] == 4
        assert rows.tobytes() == want and len(want) > 16 * 1000, (tag, i, rows.shape, len(want) // 16)
        assert nonzero[i] == (points if status[i] == 0 else 0), (tag, i)
        out.append((rows, points))
    return out


@pytest.mark.parametrize("lidar", sorted(LIDARS))
@pytest.mark.parametrize("uniform", [True, False])
@pytest.mark.parametrize("method", ["rans", "lz4", "bzip2"])
def test_decompress_rows_equals_the_per_frame_path(env, tmp_path, method, uniform, lidar):
    M, T = 20, _T(env, lidar)
    blobs = _containers(env, lidar, M, uniform, method)
    bd = env["pl"].BatchDecompressor(T, M, 2 * ACC, uniform=uniform, level_acc=LACC, basic_compressor=method)
    got = _check(env, tmp_path, bd, blobs, T, M, 2 * ACC, LACC, uniform, method, tag=(method, uniform, lidar))
    # the device form: the frames back to back, nothing else in the rows; more than one chunk packs behind the chunk before
    class Two(env["pl"].BatchDecompressor):
        CHUNK_FRAMES = 2
    if method == "rans" and uniform:
        five = [blobs[k % 2] for k in (0, 1, 1, 0, 1)]
        small = Two(T, M, 2 * ACC, uniform=uniform, level_acc=LACC, basic_compressor=method)
        assert small.chunk == 2
        status, offsets, rows, nonzero = small.decompress_rows_device(five)
        assert status.cpu().tolist() == [0] * 5 and rows.shape == (5 * T.H * T.W, 4)
        off = offsets.cpu().numpy()
        assert off[0] == 0 and np.diff(off).tolist() == [got[k % 2][0].shape[0] for k in (0, 1, 1, 0, 1)]
        host = rows[: int(off[-1])].cpu().numpy()
        for i, k in enumerate((0, 1, 1, 0, 1)):
            assert host[off[i]: off[i + 1]].tobytes() == got[k % 2][0].tobytes() and int(nonzero[i]) == got[k % 2][1], i
        assert small.decompress_rows([]) == []


def test_reference_bitstream_once(env, tmp_path):
    """The .rpcc bytes the reference wrote for its example sweep (bzip2, uniform, 100 clusters): 94 053 rows, the file of the per-frame path."""
    z = np.load(os.path.join(HERE, "golden", "example_64E.npz"))
    blob, T = z["rpcc"].tobytes(), _T(env, "Velodyne64E")
    bd = env["pl"].BatchDecompressor(T, 100, 2 * ACC, basic_compressor="bzip2")
    got = _check(env, tmp_path, bd, [blob], T, 100, 2 * ACC, LACC, True, "bzip2", tag="example_64E")
    assert got[0][0].shape == (z["q_uniform"].shape[0], 4) and not got[0][0][:, 3].any()


def test_uint16_labels(env, tmp_path):
    M, T = 300, _T(env, "VelodyneVLP16")
    blobs = _containers(env, "VelodyneVLP16", M, True, "bzip2")
    bd = env["pl"].BatchDecompressor(T, M, 2 * ACC, basic_compressor="bzip2")
    assert bd.rows_buffers(1)[1].dtype == env["torch"].uint16
    _check(env, tmp_path, bd, blobs, T, M, 2 * ACC, LACC, True, "bzip2", tag="uint16")


def test_dbscan_stream_with_max_labels(env, tmp_path):
    from rpcc_amd.utils import load_compressor_cfg
    T = _T(env, "VelodyneVLP16")
    cfg = load_compressor_cfg(os.path.join(os.path.dirname(HERE), "r-pcc_amd", "cfgs", "compressor.yaml"))
    bc = env["pl"].BatchCompressor(T, cluster_num=100, accuracy=ACC, uniform=True, model_method="point", compressor_cfg=dict(cfg), basic_compressor="bzip2",
                                   seed=7, segment_method="DBSCAN", DBSCAN_eps=1.5)
    blobs = bc.compress(_frames(env, "VelodyneVLP16"), frame_ids=[11, 12])
    cu = env["cu"]
    bz = cu.BasicCompressor(method_name="bzip2")
    rows = [len(bz.decompress_dict(cu.unpack_bitstream(b, uniform=True))["plane_param"]) // 16 for b in blobs]
    for cap in (1023, max(rows) - 1):        # the second: the frame with the most model rows goes through the per-frame fallback
        bd = env["pl"].BatchDecompressor(T, None, 2 * ACC, max_labels=cap)
        _check(env, tmp_path, bd, blobs, T, None, 2 * ACC, None, True, "bzip2", tag=("DBSCAN", cap))


def test_intensity_fills_the_fourth_column(env, tmp_path):
    M, T = 20, _T(env, "VelodyneVLP16")
    rng = np.random.default_rng(21)
    frames = [np.ascontiguousarray(np.concatenate([f[:, :3], (rng.integers(0, 100, f.shape[0]) / np.float32(100))[:, None]], 1), dtype=np.float32)
              for f in _frames(env, "VelodyneVLP16")]
    for method in ("rans", "bzip2"):
        blobs = env["pl"].BatchCompressor(T, cluster_num=M, accuracy=ACC, basic_compressor=method, seed=4, intensity_scale=100.0).compress(frames)
        bd = env["pl"].BatchDecompressor(T, M, 2 * ACC, basic_compressor=method, intensity=True)
        got = _check(env, tmp_path, bd, blobs, T, M, 2 * ACC, None, True, method, intensity=True, tag=("intensity", method))
        assert all(r[:, 3].any() for r, _ in got)
        # the same containers without asking: +0.0 in the fourth column, the same first three
        bare = env["pl"].BatchDecompressor(T, M, 2 * ACC, basic_compressor=method).decompress_rows(blobs)
        for (r, _), b in zip(got, bare):
            assert not b.view(np.uint32)[:, 3].any() and b[:, :3].tobytes() == r[:, :3].tobytes()


# ------------------------------------------------------------------------------------------------
# 3. fallback and refusal
# ------------------------------------------------------------------------------------------------
def _trailing_byte(env, blob):
    d = dict(env["cu"].unpack_bitstream(blob, True))
    d["plane_param"] = d["plane_param"] + b"\x00"      # bz2.decompress ignores it, the device decoder refuses the stream
    return env["cu"].pack_bitstream(d, True)


def test_chunk_with_fallback_and_refusal(env, tmp_path):
    M, T = 20, _T(env, "VelodyneVLP16")
    blobs = _containers(env, "VelodyneVLP16", M, True, "bzip2")
    odd = _trailing_byte(env, blobs[1])
    bd = env["pl"].BatchDecompressor(T, M, 2 * ACC, basic_compressor="bzip2")
    status, offsets, rows, nonzero = bd.decompress_rows_device([blobs[0], odd, blobs[0]])
    assert status.cpu().tolist() == [0, env["lib"].STREAM_E_ENTROPY, 0]
    off = offsets.cpu().numpy()
    assert off[1] == off[2] and off[3] == 2 * off[1] and int(nonzero[1]) == 0          # the refused frame has no rows on the device
    clean = _check(env, tmp_path, bd, blobs, T, M, 2 * ACC, LACC, True, "bzip2")
    got = bd.decompress_rows([blobs[0], odd, blobs[0]])
    for r, k in zip(got, (0, 1, 0)):
        assert r.tobytes() == clean[k][0].tobytes(), k
    assert bd.rows_fallback(odd, 1)[1] == clean[1][1]          # the point count --output prints for a frame of the fallback
    other = _containers(env, "Velodyne32E", M, True, "bzip2")[0]
    with pytest.raises(ValueError, match=r"frame 1\b"):
        bd.decompress_rows([blobs[0], other, blobs[1]])


# ------------------------------------------------------------------------------------------------
# 4. StreamingDecompressor and the tool
# ------------------------------------------------------------------------------------------------
def _tree(root):
    return {os.path.relpath(os.path.join(d, f), root): open(os.path.join(d, f), "rb").read() for d, _, fs in os.walk(root) for f in fs}


def test_streaming_decompressor_and_tool(env, tmp_path, capsys):
    from rpcc_amd.tools import compress as tc
    from rpcc_amd.tools import decompress_datalist as tdl
    M, T, lidar = 20, _T(env, "VelodyneVLP16"), "VelodyneVLP16"

    class Two(env["pl"].BatchDecompressor):
        CHUNK_FRAMES = 2

    gd = env["orc"].GEOMS[lidar]
    frames = [env["synth"].make_frame(7400 + i, gd["H"], gd["W"], vmax_deg=gd["vmax_deg"], vmin_deg=gd["vmin_deg"]).numpy() for i in range(5)]
    blobs = env["pl"].BatchCompressor(T, cluster_num=M, accuracy=ACC, basic_compressor="rans", seed=3).compress(frames)
    blobs[2] = _containers(env, lidar, M, True, "rans")[0]
    src = tmp_path / "in"
    names = []
    for k, b in enumerate(blobs):                      # 2 * chunk + 1 files, in two directories
        p = src / ("seq%d" % (k % 2)) / ("sweep%03d.rpcc" % k)
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_bytes(b)
        names.append(str(p))
    (tmp_path / "list.txt").write_text("\n".join(names) + "\n")
    base = ["--datalist", str(tmp_path / "list.txt"), "--lidar", lidar, "--basic_compressor", "rans", "--cluster_num", str(M), "--accuracy", str(ACC)]
    parse = lambda out, *flags: tc.make_parser(datalist=True).parse_args(base + ["--output_dir", str(tmp_path / out)] + list(flags))
    # the files of the existing --batch_decode path
    tdl.decompress(parse("batch", "--batch_decode", "--output"))
    lines = capsys.readouterr().out.splitlines()
    want = _tree(tmp_path / "batch")
    assert len(want) == 5 and len(set(want.values())) == 5 and all(len(v) > 16000 for v in want.values())
    # the class, two frames per chunk, two chunks in flight
    bd = Two(T, M, 2 * ACC, basic_compressor="rans")
    assert bd.chunk == 2
    sd = env["loader"].StreamingDecompressor(bd, depth=2, workers=2)
    a = parse("stream")
    seen = []
    assert sd.run(names, [tdl.output_path(a, n) for n in names], on_frame=lambda i, rows, nz: seen.append((i, rows, nz))) == 5
    assert _tree(tmp_path / "stream") == want                      # names, directories, bytes
    assert [s[0] for s in seen] == list(range(5)) and [16 * s[1] for s in seen] == [len(want[os.path.relpath(tdl.output_path(a, n), tmp_path / "stream")]) for n in names]
    assert sd.run([], []) == 0 and _tree(tmp_path / "stream") == want
    # depth 1 and 3 write the same
    for depth in (1, 3):
        a = parse("stream%d" % depth)
        env["loader"].StreamingDecompressor(bd, depth=depth, workers=2).run(names, [tdl.output_path(a, n) for n in names])
        assert _tree(tmp_path / ("stream%d" % depth)) == want, depth
    # the tool: the same files and the same --output lines, but for the directory
    tdl.decompress(parse("tool", "--stream_decode", "--output"))
    out = capsys.readouterr().out.splitlines()
    assert _tree(tmp_path / "tool") == want
    assert [ln.replace(str(tmp_path / "tool"), "D") for ln in out] == [ln.replace(str(tmp_path / "batch"), "D") for ln in lines] and len(out) == 5
    # a refused file in the second chunk: named; the first chunk's files complete, none for the refused frame or those behind it
    bad = src / "seq1" / "sweep003.rpcc"
    bad.write_bytes(_containers(env, "Velodyne32E", M, True, "rans")[0])
    a = parse("refused")
    outs = [tdl.output_path(a, n) for n in names]
    with pytest.raises(ValueError, match="sweep003"):
        sd.run(names, outs)
    got = _tree(tmp_path / "refused")
    rel = [os.path.relpath(o, tmp_path / "refused") for o in outs]
    assert got[rel[0]] == want[rel[0]] and got[rel[1]] == want[rel[1]] and rel[3] not in got and rel[4] not in got
    assert all(got[k] == want[k] for k in got)
    # the slots are free again: the same object decodes the sound list afterwards
    bad.write_bytes(blobs[3])
    a = parse("again")
    assert sd.run(names, [tdl.output_path(a, n) for n in names]) == 5 and _tree(tmp_path / "again") == want
