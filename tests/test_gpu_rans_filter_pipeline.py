"""-m gpu: basic_compressor 'rans' with rans_delta (format version 2 on the residual stream) through the batch pipelines and the tools.
On three synthetic VLP-16 sweeps (16 x 1800), uniform and non-uniform: the batch compressor's containers are the per-frame path's
(compress_point_cloud + pack_bitstream with BasicCompressor(rans_delta=True)) byte for byte, only the residual stream is an 'RB' stream,
and with the flag off the containers are those built without the argument; the batch decompressor and decode_frame read them with no flag
and return what they return for the unfiltered containers.  On the example sweep (64 x 2000): tools/compress.py --rans_delta and
tools/decompress.py round-trip it, and the filtered container is at most 0.45 of the unfiltered one."""
import os
import re
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import rans_filter_ref as F  # noqa: E402
import rans_ref as R  # noqa: E402

ACC = 0.02
LACC = np.array([2 * ACC] * 4) + np.array((0, 0.02, 0.04, 0.06))
GEOM = "VelodyneVLP16"
M = 40
WIDTHS = {"salience_level": 1, "contour_map": 1, "idx_sequence": 2, "plane_param": 4, "residual_quantized": 2}


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available()
    import __graft_entry__ as ge
    ge.build()
    from oracle import oracle as orc
    from rpcc_amd import compress_utils, dataset, pipeline, synth
    from rpcc_amd.tools.decompress import decode_frame
    gd = orc.GEOMS[GEOM]
    frames = [synth.make_frame(8100 + i, gd["H"], gd["W"], vmax_deg=gd["vmax_deg"], vmin_deg=gd["vmin_deg"]).numpy() for i in range(3)]
    T = dataset.build_dataset(lidar_type=GEOM).PCTransformer
    return dict(torch=torch, cu=compress_utils, pl=pipeline, dec=decode_frame, T=T, frames=frames, cache={})


def _containers(env, uniform, method, **flags):
    key = (uniform, method, tuple(sorted(flags.items())))
    if key not in env["cache"]:
        bc = env["pl"].BatchCompressor(env["T"], cluster_num=M, accuracy=ACC, uniform=uniform, basic_compressor=method, seed=4, **flags)
        env["cache"][key] = bc.compress(env["frames"])
    return env["cache"][key]


@pytest.mark.parametrize("uniform", [True, False], ids=["uniform", "nonuniform"])
def test_batch_containers_equal_the_per_frame_path(env, uniform):
    """The per-frame path is fed from the same batch's bzip2 containers, as in tests/test_gpu_rans_pipeline.py."""
    cu, T = env["cu"], env["T"]
    got = _containers(env, uniform, "rans", rans_delta=True)
    plain = _containers(env, uniform, "rans")
    assert _containers(env, uniform, "rans", rans_delta=False) == plain          # the flag off: the containers built without the argument
    delta, bz = cu.BasicCompressor(method_name="rans", rans_delta=True), cu.BasicCompressor(method_name="bzip2")
    assert cu.BasicCompressor(method_name="bzip2", rans_delta=True).batch_codec() is None      # the flag does nothing with another method
    for b, (g, w) in enumerate(zip(got, _containers(env, uniform, "bzip2"))):
        cd = cu.unpack_bitstream(w, uniform=uniform)
        rows = len(bz.decompress(cd["plane_param"])) // 16
        rq, idx_map, sal, plane = cu.decompress_point_cloud(cd, bz, rows, T.H, T.W)
        original, compressed = cu.compress_point_cloud(delta, plane, idx_map, sal, rq)
        assert g == cu.pack_bitstream(compressed, uniform=uniform), (uniform, b)
        assert g == cu.pack_frames(delta, [original], uniform=uniform)[0], (uniform, b)
        streams, before = cu.unpack_bitstream(g, uniform=uniform), cu.unpack_bitstream(plain[b], uniform=uniform)
        assert len(streams) == (4 if uniform else 5)
        for k, s in streams.items():              # each stream is the reference's of that array: the filter on the residuals alone
            filt = F.FILTER_DELTA if k == "residual_quantized" else F.FILTER_NONE
            assert s[3] == WIDTHS[k] and s == F.encode(original[k].tobytes(), WIDTHS[k], filter=filt), (uniform, b, k)
            assert (s == before[k]) == (k != "residual_quantized"), (uniform, b, k)
        assert streams["residual_quantized"][:3] == b"RB\x01" and len(streams["residual_quantized"]) < len(before["residual_quantized"])
        assert delta.compress(original["residual_quantized"]) == streams["residual_quantized"]
        assert delta.decompress(streams["residual_quantized"]) == original["residual_quantized"].tobytes()


@pytest.mark.parametrize("uniform", [True, False], ids=["uniform", "nonuniform"])
def test_decoders_read_both_versions_without_a_flag(env, uniform):
    cu, T = env["cu"], env["T"]
    blobs, plain = _containers(env, uniform, "rans", rans_delta=True), _containers(env, uniform, "rans")
    bd = env["pl"].BatchDecompressor(T, M, 2 * ACC, uniform=uniform, level_acc=LACC, basic_compressor="rans")
    got, want = bd.decompress(blobs), bd.decompress(plain)
    mixed = bd.decompress([blobs[0], plain[1], blobs[2]])             # both versions in one call
    for b, blob in enumerate(blobs):
        ref = env["dec"](cu.unpack_bitstream(blob, uniform), cu.BasicCompressor(method_name="rans"), T, M, 2 * ACC, LACC, uniform)
        for name, x, y, z, m in zip(("rec", "pc", "seg"), got[b], ref, want[b], mixed[b]):
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() == z.tobytes() == m.tobytes(), (uniform, b, name)
        assert int((ref[2] > 1).sum()) > 0


def test_tools_round_trip_the_example_sweep_and_the_container_shrinks(env, tmp_path, capsys):
    from rpcc_amd.tools import compress as tc
    from rpcc_amd.tools import decompress as td
    xyz = np.load(os.path.join(HERE, "golden", "example_64E.npz"))["xyz"]
    src = tmp_path / "frame.bin"
    np.concatenate((xyz[:, :3], np.zeros((xyz.shape[0], 1), np.float32)), 1).astype(np.float32).tofile(src)
    recs, errs, size = {}, {}, {}
    for m, extra in (("plain", []), ("delta", ["--rans_delta"])):
        out, rec = tmp_path / ("frame_%s.rpcc" % m), tmp_path / ("rec_%s.npy" % m)
        capsys.readouterr()
        tc.compress(tc.make_parser().parse_args(["--input", str(src), "--output", str(out), "--eval", "--lidar", "Velodyne64E",
                                                 "--basic_compressor", "rans"] + extra))
        text = capsys.readouterr().out
        errs[m] = float(re.search(r"^    Depth Error \(max\): +([0-9.eE+-]+)", text, re.M).group(1))
        td.decompress(td.make_parser().parse_args(["--input", str(out), "--output", str(rec), "--lidar", "Velodyne64E", "--basic_compressor", "rans"]))
        recs[m], size[m] = np.load(rec), os.path.getsize(out)
    print("container bytes:", size, "ratio %.4f" % (size["delta"] / size["plain"]), "Depth Error (max):", errs)
    assert np.array_equal(recs["plain"], recs["delta"]) and errs["plain"] == errs["delta"] <= ACC + 1e-4
    streams = env["cu"].read_compressed_bitstream(str(tmp_path / "frame_delta.rpcc"))
    assert [v[:2] for v in streams.values()] == [b"RA", b"RA", b"RA", b"RB"] and all(F.decode(v)[0] == R.OK for v in streams.values())
    assert size["delta"] <= 0.45 * size["plain"]
