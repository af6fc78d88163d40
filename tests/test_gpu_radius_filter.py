"""Radius outlier removal on the MI355X (librpcc_filter.so, rpcc_amd.outlier): every case of tests/filter_cases.py against the numpy
reference (tests/radius_filter_ref.py), the pruned search against brute force bit for bit, repeats, the caller-buffer contract, and the
front ends: the dataset, remove_radius_outlier, pipeline.BatchCompressor and the streaming loader against the host-compacted frames."""
import os

import numpy as np
import pytest

import buffer_arena as BA
import filter_cases as FC
import radius_filter_ref as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def env():
    import torch
    import __graft_entry__ as ge
    ge.build()
    from rpcc_amd import _filter_lib, _lib, outlier, pipeline, synth
    from rpcc_amd.dataset import build_dataset
    assert torch.cuda.is_available()
    return dict(torch=torch, F=_filter_lib, lib=_lib, outlier=outlier, pl=pipeline, synth=synth, build_dataset=build_dataset, dev=torch.device("cuda:0"))


def dev(env, a):
    return env["torch"].from_numpy(np.ascontiguousarray(a)).to(env["dev"])


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def run(env, case, brute=False, ws=None):
    xyz, offsets, nb, radius = case
    r = env["outlier"].radius_outlier_mask(dev(env, xyz), dev(env, offsets), nb, radius, brute_force=brute, stats=True, masked=True, ws=ws)
    env["torch"].cuda.synchronize()
    return {k: getattr(r, k).cpu().numpy() for k in r._fields}


def same(a, b, tag, fields=("keep", "count", "kept", "masked")):
    for k in fields:
        assert np.array_equal(bits(a[k]), bits(b[k])), (tag, k)


def check(env, case, tag=""):
    """keep, count and kept equal the reference, pruned and brute force; pruned equals brute force bit for bit, masked included; a repeat
    run is identical.  -> the pruned result and the reference."""
    ref = R.radius_filter(*case)
    ref["masked"] = R.masked(case[0], ref["keep"])
    pruned, again, brute = run(env, case), run(env, case), run(env, case, brute=True)
    for got, name in ((pruned, "pruned"), (brute, "brute")):
        same(got, ref, (tag, name))
    same(pruned, brute, (tag, "pruned vs brute"))
    same(pruned, again, (tag, "repeat"))
    for b in range(len(case[1]) - 1):      # brute force tests every ordered pair of finite points of the frame
        f = int(np.isfinite(case[0][case[1][b]:case[1][b + 1], :3]).all(1).sum())
        assert brute["stats"][b, 0] == f * f, (tag, b)
    return pruned, ref


# ---- frame sizes -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", FC.FRAME_SIZES)
def test_single_frames(env, n):
    check(env, FC.single_frame(n)[0], n)


def test_mixed_batch_and_each_frame_alone(env):
    case, _ = FC.mixed_batch()
    xyz, offsets, nb, radius = case
    got, _ = check(env, case, "batch")
    for b in range(len(offsets) - 1):
        lo, hi = int(offsets[b]), int(offsets[b + 1])
        alone, _ = check(env, (xyz[lo:hi], FC.offsets_of([hi - lo]), nb, radius), ("alone", b))
        for k in ("keep", "count", "masked"):
            assert np.array_equal(bits(alone[k]), bits(got[k][lo:hi])), (b, k)
        assert alone["kept"][0] == got["kept"][b]


def test_twin_frames(env):
    case, f = FC.twin_frames()
    got, _ = check(env, case)
    assert not got["keep"][f["twins"]].any()


# ---- the keep threshold ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", FC.THRESHOLD_NB)
def test_threshold_groups(env, nb):
    case, f = FC.threshold_groups(nb)
    got, _ = check(env, case, nb)
    g = f["groups"]
    assert not got["keep"][g["below"]].any() and got["keep"][g["at"]].all() and got["keep"][g["dup"]].all() and got["keep"][g["spread"]].all()
    assert np.all(got["count"][g["dup"]] == nb + 1)      # clipped: 60 duplicates


# ---- the boundary and the screen -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", FC.BAND_RADII)
def test_band_pairs(env, radius):
    case, f = FC.band_pairs(radius)
    got, _ = check(env, case, radius)
    assert np.array_equal(got["keep"], FC.band_expected(case, f))
    for g in f["groups"]:
        assert got["count"][g["partner"]] == (4 if g["neighbour"] else 1), (g["axis"], g["step"])


# ---- far tiles and the list ------------------------------------------------------------------------------------------------------------
def test_far_tiles(env):
    case, f = FC.far_tiles()
    got, _ = check(env, case)
    assert got["keep"][f["loners"]].all() and not got["keep"][f["outlier"]]
    assert got["stats"][0, 1] >= f["tiles"]      # the outlier's lane alone has been through every tile


# ---- non-finite ------------------------------------------------------------------------------------------------------------------------
def test_nonfinite_and_both_strides(env):
    case, f = FC.nonfinite()
    rows, offsets, nb, radius = case
    got16, _ = check(env, case, "stride 16")
    got12, _ = check(env, (np.ascontiguousarray(rows[:, :3]), offsets, nb, radius), "stride 12")
    assert np.array_equal(got16["keep"], got12["keep"]) and np.array_equal(got16["count"], got12["count"])
    assert not got16["keep"][f["bad"]].any() and not got16["keep"][f["A"]].any() and got16["keep"][f["B"]].all()
    assert np.array_equal(bits(got16["masked"][:, 3]), bits(rows[:, 3]))      # intensity copied bit for bit, NaN included
    assert np.array_equal(bits(got16["masked"][:, :3]), bits(got12["masked"]))


# ---- order -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["columns", "beams"])
def test_stored_and_shuffled_order(env, name):
    xyz = FC.sweep_slices()[name]
    stored, shuffled, perm = FC.ordered_and_shuffled(xyz)
    a, _ = check(env, stored, (name, "stored"))
    b, _ = check(env, shuffled, (name, "shuffled"))
    assert np.array_equal(a["keep"][perm], b["keep"]) and np.array_equal(a["count"][perm], b["count"])
    n = xyz.shape[0]
    assert a["stats"][0, 0] < n * n      # fewer pair tests than brute force
    print("%s: %d points, pair tests stored %d, shuffled %d, brute force %d" % (name, n, a["stats"][0, 0], b["stats"][0, 0], n * n))


# ---- the whole example sweep -----------------------------------------------------------------------------------------------------------
def test_example_sweep_equals_golden(env):
    g = FC.golden()
    xyz = FC.example_sweep()
    case = (xyz, FC.offsets_of([xyz.shape[0]]), 3, 1.0)
    a, _ = check(env, case, "sweep")
    assert np.array_equal(a["keep"], g["keep"]) and int((~a["keep"]).sum()) == 283 and a["kept"][0] == g["n"] - 283
    assert np.array_equal(np.nonzero(~a["keep"])[0], g["removed"])
    assert 0 < a["stats"][0, 0] < g["n"] * g["n"]      # fewer pair tests than brute force
    print("example sweep: %d pair tests, %d tiles visited (brute force: %d pair tests)" % (a["stats"][0, 0], a["stats"][0, 1], g["n"] * g["n"]))
    filtered, index = env["outlier"].remove_radius_outlier(xyz)
    assert index.dtype == np.int64 and np.array_equal(index, np.nonzero(g["keep"])[0]) and np.array_equal(filtered, xyz[g["keep"]])
    f64, i64 = env["outlier"].remove_radius_outlier(dev(env, xyz.astype(np.float64)), nb_points=3, radius=1.0)      # a device tensor, wider dtype
    assert f64.is_cuda and f64.dtype == env["torch"].float64 and np.array_equal(i64.cpu().numpy(), index)
    assert np.array_equal(f64.cpu().numpy(), xyz[g["keep"]].astype(np.float64))


# ---- buffers ---------------------------------------------------------------------------------------------------------------------------
def test_caller_buffers(env):
    """Exact-size ws with hostile contents between guard bytes, ws at base + 16, outputs pre-filled and fully overwritten, guards intact."""
    torch, F = env["torch"], env["F"]
    from rpcc_amd._lib import ptr, stream
    case, _ = FC.mixed_batch()
    xyz, offsets, nb, radius = case
    rows = np.concatenate([xyz, np.full((xyz.shape[0], 1), 0.5, np.float32)], 1)
    ref = R.radius_filter(*case)
    total, B = xyz.shape[0], len(offsets) - 1
    nbytes = F.lib().rpcc_filter_workspace_bytes(total, B)
    assert nbytes > 0
    pts, offs = dev(env, rows), dev(env, offsets)
    for shift in (0, 16):      # the workspace at a 256-aligned address, and at base + 16
        arena = BA.Arena(nbytes + shift, device=env["dev"])
        for pattern in ("nan", "ones", "intmax", "alt(0,1)", "half(0)"):
            arena.fill(pattern)
            ws = arena.view[shift:]
            assert ws.numel() == nbytes and ws.data_ptr() % 256 == shift
            head = arena.view[:shift].clone()

            def call(fill):
                out = dict(keep=BA.filled((total,), torch.uint8, env["dev"], fill), count=BA.filled((total,), torch.int32, env["dev"], fill),
                           kept=BA.filled((B,), torch.int64, env["dev"], fill), masked=BA.filled((total, 4), torch.float32, env["dev"], fill),
                           stats=BA.filled((B, 2), torch.int64, env["dev"], fill))
                F.check(F.lib().rpcc_filter_radius(ptr(pts), 16, ptr(offs), total, B, radius, nb, 0, ptr(out["keep"]), ptr(out["count"]), ptr(out["kept"]),
                                                   ptr(out["masked"]), ptr(out["stats"]), ptr(ws), stream()))
                torch.cuda.synchronize()
                assert bool((out["stats"] >= 0).all()) and bool((out["stats"] < total * total).all())      # written (0x00.. / 0xFF.. are 0 / -1): it
                out.pop("stats")                                                                           # counts work and may differ between runs
                return out
            got = {}
            holes = BA.unwritten(call, got)
            assert all(not h.any() for h in holes.values()), (pattern, shift, {k: int(h.sum()) for k, h in holes.items()})
            assert arena.check_guards() is None and torch.equal(arena.view[:shift], head), (pattern, shift)
            assert np.array_equal(got["keep"].cpu().numpy().astype(bool), ref["keep"]) and np.array_equal(got["count"].cpu().numpy(), ref["count"])
            assert np.array_equal(got["kept"].cpu().numpy(), ref["kept"])
            assert np.array_equal(bits(got["masked"].cpu().numpy()), bits(R.masked(rows, ref["keep"])))


# ---- front ends ------------------------------------------------------------------------------------------------------------------------
def test_dataset_filters_before_the_projection(env, tmp_path):
    """Fails with NotImplementedError before librpcc_filter.so existed."""
    xyz = FC.example_sweep()
    g = FC.golden()
    rows = np.concatenate([xyz, np.zeros((xyz.shape[0], 1), np.float32)], 1)
    rows.tofile(str(tmp_path / "sweep.bin"))
    (tmp_path / "list.txt").write_text(str(tmp_path / "sweep.bin") + "\n")
    ds = env["build_dataset"](str(tmp_path / "list.txt"), lidar_type="Velodyne64E", use_radius_outlier_removal=True)
    point_cloud, range_image, original, name = ds[0]
    want = np.expand_dims(ds.PCTransformer.point_cloud_to_range_image(xyz[g["keep"]]), -1)      # the host-compacted cloud
    assert np.array_equal(bits(range_image), bits(want)) and name == str(tmp_path / "sweep.bin")
    assert np.array_equal(bits(point_cloud), bits(ds.PCTransformer.range_image_to_point_cloud(want)))
    assert np.array_equal(bits(np.ascontiguousarray(original)), bits(xyz))                      # unfiltered
    plain = env["build_dataset"](str(tmp_path / "list.txt"), lidar_type="Velodyne64E")
    assert not np.array_equal(bits(plain[0][1]), bits(range_image))                             # the filter shows in the image
    unfiltered = ds.load_range_image_points_from_file(name)                                     # stays unfiltered, as in the reference
    assert np.array_equal(bits(unfiltered[1]), bits(plain[0][1]))


def vlp16_frames(env, n, seed=300):
    """Synthetic VLP-16 sweeps with 60 stray points each, thrown between the sensor and the scene."""
    from oracle import oracle as orc
    gd = orc.GEOMS["VelodyneVLP16"]
    rng = np.random.default_rng(seed)
    frames = []
    for i in range(n):
        f = env["synth"].make_frame(seed + i, gd["H"], gd["W"], vmax_deg=gd["vmax_deg"], vmin_deg=gd["vmin_deg"]).numpy()
        k = rng.choice(f.shape[0], 60, replace=False)
        f = f.copy()
        f[k] *= rng.uniform(0.3, 0.7, (60, 1)).astype(np.float32)
        frames.append(f)
    return frames


def compacted(frames):
    out = [f[R.radius_filter(f, None, 3, 1.0)["keep"]] for f in frames]
    assert all(0 < c.shape[0] < f.shape[0] for c, f in zip(out, frames))
    return out


@pytest.mark.parametrize("segment_method", ["FPS", "DBSCAN"])
def test_batch_compressor_equals_host_compaction(env, segment_method):
    ds = env["build_dataset"](lidar_type="VelodyneVLP16")
    frames = vlp16_frames(env, 3)
    kw = dict(accuracy=0.02, seed=7, segment_method=segment_method, DBSCAN_eps=1.5)
    plain = env["pl"].BatchCompressor(ds.PCTransformer, **kw)
    want = plain.compress(compacted(frames), frame_ids=[4, 5, 6])
    assert want != plain.compress(frames, frame_ids=[4, 5, 6])      # the stray points show in the containers
    got = env["pl"].BatchCompressor(ds.PCTransformer, radius_outlier_removal=(3, 1.0), **kw).compress(frames, frame_ids=[4, 5, 6])
    assert got == want


def test_streaming_loader_rows_equals_host_compaction(env):
    from rpcc_amd.loader import StreamingCompressor
    ds = env["build_dataset"](lidar_type="VelodyneVLP16")
    frames = vlp16_frames(env, 3, seed=340)
    rows = [np.concatenate([f, np.full((f.shape[0], 1), np.nan, np.float32)], 1) for f in frames]      # NaN intensity: never interpreted
    ids = [11, 12, 13]
    want = env["pl"].BatchCompressor(ds.PCTransformer, accuracy=0.02, seed=7).compress(compacted(frames), frame_ids=ids)
    bc = env["pl"].BatchCompressor(ds.PCTransformer, accuracy=0.02, seed=7, radius_outlier_removal=(3, 1.0))
    for ingest, src in (("rows", rows), ("xyz", frames)):
        got = {}
        n = StreamingCompressor(bc, batch=3, depth=2, workers=2, ingest=ingest).run([(src, ids)], sink=lambda k, r: got.__setitem__(k, r))
        assert n == 3 and [b for k in sorted(got) for b in got[k]] == want, ingest


def test_mixed_batch_compressor_refuses_the_option(env):
    ds = env["build_dataset"](lidar_type="VelodyneVLP16")
    with pytest.raises(NotImplementedError, match="radius_outlier_removal"):
        env["pl"].MixedBatchCompressor({"VelodyneVLP16": ds.PCTransformer}, radius_outlier_removal=(3, 1.0))
    env["pl"].MixedBatchCompressor({"VelodyneVLP16": ds.PCTransformer})


def test_tools_with_the_flag_equal_the_tools_on_host_compacted_files(env, tmp_path):
    """tools/compress.py (filters per frame through the dataset) and tools/compress_datalist.py (the batch front-end, both ingest modes) with
    --use_radius_outlier_removal write the files they write without it for the host-compacted sweeps of the same base names (the frame
    identity of the seeded plane fits is the base name)."""
    from rpcc_amd.tools import compress as tc, compress_datalist as cd
    frames = vlp16_frames(env, 2, seed=380)
    names = {}
    for kind, fs in (("raw", frames), ("host", compacted(frames))):
        (tmp_path / kind).mkdir()
        names[kind] = []
        for i, f in enumerate(fs):
            names[kind].append(str(tmp_path / kind / ("%06d.bin" % i)))
            np.concatenate((f, np.full((f.shape[0], 1), 0.5, np.float32)), 1).astype(np.float32).tofile(names[kind][-1])
        (tmp_path / (kind + ".txt")).write_text("\n".join(names[kind]) + "\n")
    common = ["--lidar", "VelodyneVLP16", "--seed", "3"]
    assert tc.make_parser().parse_args([]).use_radius_outlier_removal is False and tc.make_parser(datalist=True).parse_args([]).use_radius_outlier_removal is False

    def single(src, flag):
        out = str(tmp_path / "single.rpcc")
        tc.compress(tc.make_parser().parse_args(["--input", src, "--output", out] + common + flag))
        return open(out, "rb").read()
    for raw, host in zip(names["raw"], names["host"]):
        want = single(host, [])
        assert single(raw, ["--use_radius_outlier_removal"]) == want and single(raw, []) != want

    def datalist(kind, flag, tag):
        out = str(tmp_path / ("out_" + tag))
        cd.compress(tc.make_parser(datalist=True).parse_args(["--datalist", str(tmp_path / (kind + ".txt")), "--output_dir", out, "--batch", "2", "--workers", "2"]
                                                             + common + flag))
        return [open(cd.output_path_for(out, n), "rb").read() for n in names[kind]]
    want = datalist("host", [], "host")
    for ingest in ("rows", "xyz"):
        assert datalist("raw", ["--use_radius_outlier_removal", "--ingest", ingest], ingest) == want, ingest
    assert datalist("raw", [], "plain") != want
