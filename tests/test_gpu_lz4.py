"""-m gpu: librpcc_lz4.so against tests/lz4_ref.py byte for byte, its decoder on our streams, the
reference encoder's and liblz4's, its status codes on malformed input, and basic_compressor 'lz4' through the batch pipeline
and the tools."""
import bz2
import os
import struct
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import lz4_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def codec():
    import torch
    assert torch.cuda.is_available()
    import __graft_entry__ as ge
    ge.build()
    from rpcc_amd import lz4_codec
    return lz4_codec


def golden_arrays():
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import gen_golden_lz4
    return gen_golden_lz4.arrays()


def edge_inputs():
    rng = np.random.default_rng(7)
    out = {"len%d" % n: rng.integers(0, 4, n, dtype=np.uint8).tobytes() for n in (0, 1, 12, 13, 14, 65535, 65536, 65537)}
    out["random"] = rng.integers(0, 256, 70000, dtype=np.uint8).tobytes()
    out["zeros_600k"] = bytes(600000)
    out["big_mixed"] = (rng.integers(0, 3, 700000, dtype=np.uint8) * 85).tobytes()   # > 512 KB, compressible
    a = bytearray(rng.integers(0, 256, 1000, dtype=np.uint8).tobytes())
    a[700: 700 + 40] = a[100: 140]
    out["runs"] = bytes(a) + bytes(270) + b"ab" * 300 + bytes(14) + rng.integers(0, 256, 269, dtype=np.uint8).tobytes() + bytes(64)
    far = np.zeros(70000, np.uint8)
    far[100:120] = rng.integers(1, 256, 20, dtype=np.uint8)
    far[65535 + 100: 65535 + 120] = far[100:120]           # a match at offset exactly 65535
    out["offset_65535"] = far.tobytes()
    return out


def test_encode_golden_equals_reference(codec):
    src = golden_arrays()
    got = codec.dumps_many(list(src.values()))
    for (k, s), g in zip(src.items(), got):
        assert g == R.dumps(s), k
        assert R.loads(g) == s, k


def test_encode_edges_equal_reference(codec):
    src = edge_inputs()
    got = codec.dumps_many(list(src.values()))
    for (k, s), g in zip(src.items(), got):
        assert g == R.dumps(s), k
    assert codec.dumps(b"") == b"\0\0\0\0\0"


def test_encode_large_batch_in_one_launch(codec):
    rng = np.random.default_rng(11)
    srcs = []
    for i in range(1200):
        n = int(rng.choice([0, 5, 13, 100, 1000, 5000, 20000]))
        alpha = int(rng.integers(1, 256))
        srcs.append(rng.integers(0, alpha, n, dtype=np.uint8).tobytes())
    got = codec.dumps_many(srcs)
    for s, g in zip(srcs, got):
        assert g == R.dumps(s)
    assert codec.loads_many(got) == srcs


def test_decode_own_reference_and_liblz4_streams(codec):
    src = dict(golden_arrays(), **edge_inputs())
    own = codec.dumps_many(list(src.values()))
    assert codec.loads_many(own) == list(src.values())
    assert codec.loads_many([R.dumps(s) for s in src.values()]) == list(src.values())
    foreign = np.load(os.path.join(HERE, "golden", "lz4_foreign.npz"))
    gold = golden_arrays()
    blobs = [foreign[k].tobytes() for k in gold]
    assert codec.loads_many(blobs) == list(gold.values())
    assert codec.loads(b"\0\0\0\0") == b""


def test_decode_malformed_status(codec):
    """Malformed input is reported per stream, nothing outside the given ranges is touched and the other streams decode."""
    from rpcc_amd import _lz4_lib as L
    s = golden_arrays()["contour_map"]
    good = R.dumps(s)
    blk = good[4:]
    n = len(s)
    hdr = lambda m: struct.pack("<I", m)
    cases = {
        "truncated": (good[: len(good) // 2], L.E_TRUNCATED),
        "truncated_header": (good[:3], L.E_TRUNCATED),
        "offset_zero": (hdr(8) + bytes([0x10, 0x41, 0x00, 0x00]) + bytes([0x30]) + b"abc", L.E_OFFSET),
        "offset_past_start": (hdr(20) + bytes([0x10, 0x41, 0x02, 0x00]) + bytes([0x50]) + b"abcde", L.E_OFFSET),
        "header_too_small": (hdr(n - 1) + blk, L.E_OVERRUN),
        "header_too_large": (hdr(n + 1) + blk, L.E_SIZE),
        "trailing_garbage": (good + b"\x1f\x01\x00", L.E_OVERRUN),
        "empty_block": (hdr(5), L.E_TRUNCATED),
    }
    blobs = [b for b, _ in cases.values()] + [good]
    st, outs = codec.decode_many(blobs)
    for (k, (_, want)), got in zip(cases.items(), st[:-1]):
        assert got == want, k
    assert st[-1] == 0 and outs[-1] == s
    with pytest.raises(ValueError):
        codec.loads(cases["offset_zero"][0])
    # a header above the capacity the caller gave (here: what a block of this length can produce at most)
    st, _ = codec.decode_many([hdr(255 * 8 + 1) + b"\x00" * 4])
    assert st[0] == L.E_CAPACITY


def test_basic_compressor_lz4_uses_the_codec(codec):
    from rpcc_amd import compress_utils as cu
    bc = cu.BasicCompressor(method_name="lz4")
    a = np.arange(5000, dtype=np.int16) % 37
    blob = bc.compress(a)
    assert blob == R.dumps(a.tobytes())
    assert bc.decompress(blob) == a.tobytes()


def _frames(geom, k, seed):
    from oracle import oracle as orc
    from rpcc_amd import synth
    gd = orc.GEOMS[geom]
    return [synth.make_frame(seed + i, gd["H"], gd["W"], vmax_deg=gd["vmax_deg"], vmin_deg=gd["vmin_deg"]).numpy() for i in range(k)]


def _lz4_from_bzip2(blob, uniform):
    """The container the host path writes with lz4_ref as the coder, from the same frame's bzip2 container."""
    from rpcc_amd import compress_utils as cu
    d = cu.unpack_bitstream(blob, uniform=uniform)
    return cu.pack_bitstream({k: R.dumps(bz2.decompress(v)) for k, v in d.items()}, uniform=uniform)


def _dataset(geom):
    from rpcc_amd import dataset as ds
    if geom == "Velodyne64E_unofficial":
        return ds.build_dataset(dataset_name="KITTI_test")
    return ds.build_dataset(lidar_type=geom)


@pytest.mark.parametrize("geom,uniform,method,M", [
    ("Velodyne64E", True, "point", 100), ("Velodyne64E", False, "plane", 300), ("Velodyne32E", False, "point", 100),
    ("VelodyneVLP16", True, "plane", 300), ("Velodyne64E_unofficial", True, "point", 100), ("Velodyne64E_2048", False, "plane", 100)])
def test_batch_compressor_lz4_equals_host_containers(codec, geom, uniform, method, M):
    from rpcc_amd import pipeline as pl
    T = _dataset(geom).PCTransformer
    frames = _frames(geom, 3, 500) + [np.zeros((0, 3), np.float32)]
    kw = dict(cluster_num=M, accuracy=0.02, uniform=uniform, model_method=method, seed=5)
    want = pl.BatchCompressor(T, basic_compressor="bzip2", **kw).compress(frames)
    bc = pl.BatchCompressor(T, basic_compressor="lz4", **kw)
    got = bc.compress(frames)
    for b, (w, g) in enumerate(zip(want, got)):
        assert g == _lz4_from_bzip2(w, uniform), (geom, b)


def test_batch_compressor_lz4_two_batches_in_flight(codec):
    from rpcc_amd import pipeline as pl
    T = _dataset("Velodyne64E").PCTransformer
    a, b = _frames("Velodyne64E", 2, 700), _frames("Velodyne64E", 3, 800)
    kw = dict(accuracy=0.02, uniform=False, model_method="point", seed=1)
    ref = pl.BatchCompressor(T, basic_compressor="bzip2", **kw)
    want = ref.compress(b) + ref.compress(a)
    bc = pl.BatchCompressor(T, basic_compressor="lz4", **kw)
    ca, cb = bc.submit(a), bc.submit(b)
    got = bc.collect(cb) + bc.collect(ca)
    assert got == [_lz4_from_bzip2(w, False) for w in want]


def test_mixed_batch_compressor_lz4(codec):
    from rpcc_amd import pipeline as pl
    names = ["VelodyneVLP16", "Velodyne64E", "VelodyneVLP16"]
    T = {n: _dataset(n).PCTransformer for n in set(names)}
    frames = [_frames(n, 1, 900 + i)[0] for i, n in enumerate(names)]
    want = pl.MixedBatchCompressor(T, basic_compressor="bzip2", seed=2).compress(frames, names)
    got = pl.MixedBatchCompressor(T, basic_compressor="lz4", seed=2).compress(frames, names)
    assert got == [_lz4_from_bzip2(w, True) for w in want]


def test_compress_decompress_tools_lz4(codec, tmp_path, capsys):
    """tools/compress.py --basic_compressor lz4 then tools/decompress.py: the same range image as the bzip2 path; the .rpcc decodes
    with the plain-Python decoder."""
    from rpcc_amd import compress_utils as cu
    from rpcc_amd.tools import compress as tc
    from rpcc_amd.tools import decompress as td
    z = np.load(os.path.join(HERE, "golden", "example_64E.npz"))
    src = tmp_path / "frame.bin"
    np.concatenate((z["xyz"], np.zeros((z["xyz"].shape[0], 1), np.float32)), 1).astype(np.float32).tofile(src)
    recs = {}
    for m in ("bzip2", "lz4"):
        out = tmp_path / ("frame_%s.rpcc" % m)
        rec = tmp_path / ("rec_%s.npy" % m)
        capsys.readouterr()
        tc.compress(tc.make_parser().parse_args(["--input", str(src), "--output", str(out), "--eval", "--lidar", "Velodyne64E",
                                                 "--basic_compressor", m]))
        text = capsys.readouterr().out
        for label in ("Compression finished.", "    BPP: ", "    Depth Error (max): "):
            assert sum(1 for ln in text.splitlines() if ln.startswith(label)) == 1, (m, label)
        td.decompress(td.make_parser().parse_args(["--input", str(out), "--output", str(rec), "--lidar", "Velodyne64E",
                                                   "--basic_compressor", m]))
        recs[m] = np.load(rec)
        if m == "lz4":
            d = cu.read_compressed_bitstream(str(out))
            for v in d.values():
                R.loads(v)   # the plain-Python decoder reads every array
    assert np.array_equal(recs["bzip2"], recs["lz4"])
