"""-m gpu: librpcc_deflate.so against tests/deflate_ref.py byte for byte, its streams read by the
standard library's gzip, and basic_compressor 'deflate' with device_entropy through BasicCompressor, the batch pipeline and
the tools."""
import bz2
import gzip
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import deflate_cases as cases  # noqa: E402
import deflate_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def codec():
    import torch
    assert torch.cuda.is_available()
    import __graft_entry__ as ge
    ge.build()
    from rpcc_amd import deflate_codec
    return deflate_codec


def _first_difference(got, want):
    k = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    return "lengths %d / %d, first difference at byte %d" % (len(got), len(want), k)


def test_golden_equals_reference(codec):
    src = cases.golden_arrays()
    got = codec.compress_many(list(src.values()))
    for (k, s), g in zip(src.items(), got):
        assert g == cases.reference(k), (k, _first_difference(g, cases.reference(k)))
        assert gzip.decompress(g) == s, k
        assert len(g) == cases.PINNED[k], k


def test_edges_equal_reference(codec):
    src = cases.edge_inputs()
    got = codec.compress_many(list(src.values()))
    for (k, s), g in zip(src.items(), got):
        assert g == cases.reference(k), (k, _first_difference(g, cases.reference(k)))
        assert gzip.decompress(g) == s, k
    assert codec.compress(b"")[10:-8] == bytes([1, 0, 0, 0xFF, 0xFF])


def test_many_streams_in_one_launch(codec):
    rng = np.random.default_rng(11)
    srcs = []
    for i in range(1200):
        n = int(rng.choice([0, 5, 13, 100, 1000, 5000, 20000]))
        alpha = int(rng.integers(1, 256))
        srcs.append(rng.integers(0, alpha, n, dtype=np.uint8).tobytes())
    got = codec.compress_many(srcs)
    for i, (s, g) in enumerate(zip(srcs, got)):
        assert g == R.compress(s), (i, len(s))
        assert gzip.decompress(g) == s, i


def test_slot_below_bound_is_refused(codec):
    """A slot one byte below the bound gets dst_len -1; its bytes and its neighbours' are untouched, the other streams encode."""
    import torch
    from rpcc_amd import _deflate_lib as L
    from rpcc_amd._lib import ptr, stream
    rng = np.random.default_rng(3)
    srcs = [rng.integers(0, 5, 4000, dtype=np.uint8).tobytes(), rng.integers(0, 256, 3000, dtype=np.uint8).tobytes(),
            rng.integers(0, 7, 5000, dtype=np.uint8).tobytes()]
    dev = torch.device("cuda", torch.cuda.current_device())
    data = [torch.frombuffer(bytearray(s), dtype=torch.uint8).to(dev) for s in srcs]
    cap = np.array([codec.bound(len(s)) for s in srcs], np.int64)
    cap[1] -= 1
    gap = 64                                   # guard bytes between the slots
    off = np.zeros(3, np.int64)
    off[1:] = np.cumsum(cap + gap)[:-1]
    off += gap
    slots = torch.full((int(off[-1] + cap[-1] + gap),), 0xA5, dtype=torch.uint8, device=dev)
    meta = torch.tensor([[t.data_ptr() for t in data], [len(s) for s in srcs], off.tolist(), cap.tolist()], dtype=torch.int64, device=dev)
    dst_len = torch.zeros(3, dtype=torch.int64, device=dev)
    total = sum(len(s) for s in srcs)
    ws = torch.empty(L.lib().rpcc_deflate_workspace_bytes(3, total) // 8 + 1, dtype=torch.int64, device=dev)
    L.check(L.lib().rpcc_deflate_encode(ptr(meta[0]), ptr(meta[1]), 3, total, ptr(slots), ptr(meta[2]), ptr(meta[3]), ptr(dst_len), ptr(ws),
                                        stream()))
    got, h = dst_len.cpu().numpy(), slots.cpu().numpy()
    assert got[1] == L.E_CAPACITY
    keep = np.ones(h.size, bool)
    for k in (0, 2):
        assert h[off[k]: off[k] + got[k]].tobytes() == R.compress(srcs[k]), k
        keep[off[k]: off[k] + got[k]] = False
    assert (h[keep] == 0xA5).all()             # the refused slot, the guards and the slots' unused ends


def test_basic_compressor_device_entropy(codec):
    from rpcc_amd import compress_utils as cu
    bc = cu.BasicCompressor(method_name="deflate", device_entropy=True)
    a = np.arange(5000, dtype=np.int16) % 37
    blob = bc.compress(a)
    assert blob == R.compress(a.tobytes())
    assert bc.decompress(blob) == a.tobytes()
    d = {"x": a, "y": np.zeros(300, np.uint8)}
    assert bc.compress_dict(d) == {k: R.compress(v.tobytes()) for k, v in d.items()}
    assert cu.BasicCompressor(method_name="gzip", device_entropy=True).compress(a) == blob


def _frames(geom, k, seed):
    from oracle import oracle as orc
    from rpcc_amd import synth
    gd = orc.GEOMS[geom]
    return [synth.make_frame(seed + i, gd["H"], gd["W"], vmax_deg=gd["vmax_deg"], vmin_deg=gd["vmin_deg"]).numpy() for i in range(k)]


def _deflate_from_bzip2(blob, uniform):
    """The container the host path writes with deflate_ref as the coder, from the same frame's bzip2 container."""
    from rpcc_amd import compress_utils as cu
    d = cu.unpack_bitstream(blob, uniform=uniform)
    return cu.pack_bitstream({k: R.compress(bz2.decompress(v)) for k, v in d.items()}, uniform=uniform)


def _dataset(geom):
    from rpcc_amd import dataset as ds
    return ds.build_dataset(lidar_type=geom)


@pytest.mark.parametrize("geom,uniform,method,M", [("VelodyneVLP16", True, "plane", 300), ("Velodyne64E", False, "point", 100)])
def test_batch_compressor_equals_host_containers(codec, geom, uniform, method, M):
    from rpcc_amd import pipeline as pl
    T = _dataset(geom).PCTransformer
    frames = _frames(geom, 2, 500) + [np.zeros((0, 3), np.float32)]
    kw = dict(cluster_num=M, accuracy=0.02, uniform=uniform, model_method=method, seed=5)
    want = pl.BatchCompressor(T, basic_compressor="bzip2", **kw).compress(frames)
    got = pl.BatchCompressor(T, basic_compressor="deflate", device_entropy=True, **kw).compress(frames)
    for b, (w, g) in enumerate(zip(want, got)):
        assert g == _deflate_from_bzip2(w, uniform), (geom, b)


def test_batch_compressor_two_batches_in_flight(codec):
    from rpcc_amd import pipeline as pl
    T = _dataset("VelodyneVLP16").PCTransformer
    a, b = _frames("VelodyneVLP16", 1, 700), _frames("VelodyneVLP16", 2, 800)
    kw = dict(accuracy=0.02, uniform=False, model_method="point", seed=1)
    ref = pl.BatchCompressor(T, basic_compressor="bzip2", **kw)
    want = ref.compress(b) + ref.compress(a)
    bc = pl.BatchCompressor(T, basic_compressor="deflate", device_entropy=True, **kw)
    ca, cb = bc.submit(a), bc.submit(b)
    got = bc.collect(cb) + bc.collect(ca)
    assert got == [_deflate_from_bzip2(w, False) for w in want]


def test_mixed_batch_compressor(codec):
    from rpcc_amd import pipeline as pl
    names = ["VelodyneVLP16", "Velodyne64E", "VelodyneVLP16"]
    T = {n: _dataset(n).PCTransformer for n in set(names)}
    frames = [_frames(n, 1, 900 + i)[0] for i, n in enumerate(names)]
    want = pl.MixedBatchCompressor(T, basic_compressor="bzip2", seed=2).compress(frames, names)
    got = pl.MixedBatchCompressor(T, basic_compressor="deflate", device_entropy=True, seed=2).compress(frames, names)
    assert got == [_deflate_from_bzip2(w, True) for w in want]


def test_compress_decompress_tools(codec, tmp_path, capsys):
    """tools/compress.py --basic_compressor deflate --device_entropy, then tools/decompress.py --basic_compressor deflate: the same
    range image as the bzip2 path; gzip.decompress reads every array of the .rpcc."""
    from rpcc_amd import compress_utils as cu
    from rpcc_amd.tools import compress as tc
    from rpcc_amd.tools import decompress as td
    z = np.load(os.path.join(HERE, "golden", "example_64E.npz"))
    src = tmp_path / "frame.bin"
    np.concatenate((z["xyz"], np.zeros((z["xyz"].shape[0], 1), np.float32)), 1).astype(np.float32).tofile(src)
    recs = {}
    for m, extra in (("bzip2", []), ("deflate", ["--device_entropy"])):
        out = tmp_path / ("frame_%s.rpcc" % m)
        rec = tmp_path / ("rec_%s.npy" % m)
        capsys.readouterr()
        tc.compress(tc.make_parser().parse_args(["--input", str(src), "--output", str(out), "--lidar", "Velodyne64E",
                                                 "--basic_compressor", m] + extra))
        assert "Compression finished." in capsys.readouterr().out
        td.decompress(td.make_parser().parse_args(["--input", str(out), "--output", str(rec), "--lidar", "Velodyne64E",
                                                   "--basic_compressor", m]))
        recs[m] = np.load(rec)
        if m == "deflate":
            d = cu.read_compressed_bitstream(str(out))
            for k, v in d.items():
                raw = gzip.decompress(v)
                assert v == R.compress(raw), k     # the device wrote it, not gzip.compress
    assert np.array_equal(recs["bzip2"], recs["deflate"])
