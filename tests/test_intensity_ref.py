"""The intensity channel without a GPU: the two forms of the owner rule, the quantiser, payload and trailer parsing with each refusal,
the container with and without the trailer, the new entries of the C ABI (symbols, version, argument errors before the device, scratch
size), the tools' flags and the front-ends that refuse intensity."""
import ctypes
import os
import re
import struct

import numpy as np
import pytest

import intensity_cases as IC
import intensity_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW = ("rpcc_intensity_scratch_bytes", "rpcc_intensity_encode", "rpcc_intensity_decode")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    import rpcc_amd  # noqa: F401
    from rpcc_amd import _lib
    return _lib


# ---- the specification --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(IC.CASES))
def test_owner_rule_forms_agree(name):
    for batch in IC.CASES[name]():
        g = batch["g"]
        for f in batch.get("distinct", batch["frames"]):         # (a batch that repeats frames names the distinct ones)
            e = R.encode_frame(f, g, batch["scale"])
            assert np.array_equal(R.owners_closed(e["d"], e["pix"], e["ri"]), e["own"]), name
            n = int((e["ri"] != 0).sum())
            assert e["payload"].shape[0] == 8 + n and bytes(e["payload"][:4]) == b"RPI1"
            assert struct.unpack("<f", bytes(e["payload"][4:8]))[0] == np.float32(batch["scale"])
            assert np.array_equal(e["ri"].reshape(g.H, g.W).view(np.uint32), IC.orc.project(f[:, :3], g).view(np.uint32)) or name == "nonfinite"
            labels = np.where(e["ri"] != 0, 5, 1)
            back = R.decode_frame(e["payload"], labels)
            set_ = e["ri"] != 0
            w = f[e["own"][set_], 3]
            fin = np.isfinite(w) & (w >= 0) & (w * np.float32(batch["scale"]) <= 255)
            assert np.all(np.abs(back[set_][fin].astype(np.float64) - w[fin]) <= 0.5 / batch["scale"] + 1e-7), name
            assert not back[~set_].any()


def test_cases_hold_what_they_promise():
    g = IC.orc.LidarGeom(**IC.TINY)
    z = IC.zeros()[0]
    d0, pix0 = R.pixels(np.zeros((1, 3), np.float32), g)
    want = [None, 5.0, 3.0, 6.0, 5.0, None]                          # final depth of the zeros' pixel, scene by scene
    own_w = [None, .3, .4, .5, .3, None]
    for f, dep, w in zip(z["frames"], want, own_w):
        e = R.encode_frame(f, g, 255)
        assert (f[:, :3] == 0).all(1).any()
        if dep is None:
            assert e["ri"][pix0[0]] == 0 and e["own"][pix0[0]] == -1
        else:
            assert e["ri"][pix0[0]] == np.float32(dep) and f[e["own"][pix0[0]], 3] == np.float32(w)
    t = IC.ties()[0]
    e = R.encode_frame(t["frames"][0], g, 255)
    first = {}
    for i, row in enumerate(t["frames"][0]):
        first.setdefault(row[:3].tobytes(), i)
    dup_owned = [p for p in np.flatnonzero(e["own"] >= 0) if first[t["frames"][0][e["own"][p], :3].tobytes()] != e["own"][p]]
    assert not dup_owned                                                   # the first of equal rows owns
    assert len(first) < t["frames"][0].shape[0] - 30
    n = IC.nonfinite()[0]
    e = R.encode_frame(n["frames"][0], g, 255)
    assert int((e["pix"] < 0).sum()) == 7
    for col, q in zip((1, 3, 5, 7, 9, 11), (0, 255, 0, 0, 0, 255)):
        row = (0, 1, 2, 3, 0, 1)[(col - 1) // 2]
        assert e["image"][row * g.W + col] == q and abs(e["ri"][row * g.W + col] - 0.5) < 1e-6
    w = IC.wrap_clamp()[0]
    e = R.encode_frame(w["frames"][0], g, 255).copy()
    img = (e["image"].astype(np.float32) / 255).reshape(g.H, g.W)
    assert np.allclose(img[:, 0], [.11, .22, .13, .24], atol=0.5 / 255)                  # column W wraps to 0 and competes there
    assert np.allclose([img[3, 4], img[0, 4], img[3, 6], img[0, 6]], [.31, .32, .43, .44], atol=0.5 / 255)    # beyond both ends: clamped rows
    fr = IC.frames()[0]
    assert [f.shape[0] for f in fr["frames"]] == [0, 1, 63, 64, 4099]
    assert R.encode_frame(fr["frames"][0], fr["g"], 255)["payload"].shape[0] == 8


def test_past_the_grid_reaches_every_second_trip_and_the_carried_queue():
    """The batch of IC.past_the_grid(), by the reference and the launch rules alone (tests/grid_caps.py): the fill kernel and the owner pass
    make a second trip and the fix-up pass a third, and in both passes the LDS queue goes through a drain to exactly 0, a drain that
    leaves a remainder (then the tail behind the loop) and a refill after a drain.  A row counts as queued only where project_point_fast
    refuses it by rule (the reference's column is 0, the depth 0 or not finite), and as certainly fast only where it was aimed so (a
    quarter cell from a pixel centre in columns 2 .. W - 2 at 1 .. 60 m)."""
    import grid_caps as GC
    batch = IC.past_the_grid()[0]
    g, frames, which = batch["g"], batch["frames"], batch["which"]
    B, P = len(frames), g.H * g.W
    offs = IC.offsets(frames)
    total = int(offs[-1])
    assert (g.H, g.W) == (16, 512) and [f.shape[0] for f in batch["distinct"]] == [6001, 6001, 6001, 0]
    assert all(frames[b] is batch["distinct"][b % 4] for b in range(B))
    assert total >= GC.INT_OWNER_CAP * GC.INT_THREADS + 65536 and B * P > GC.INT_FILL_CAP * GC.INT_FILL_THREADS
    assert (B, total, B * P) == (247, 1116186, 2023424) or (GC.INT_OWNER_CAP, GC.INT_FILL_CAP, GC.INT_FIXUP_CAP) != (4096, 4096, 2048)
    assert GC.fill_trips(B * P, GC.INT_FILL_THREADS, GC.INT_FILL_CAP) >= 2
    assert GC.trips(total, GC.INT_THREADS, GC.INT_OWNER_CAP) >= 2 and GC.trips(total, GC.INT_THREADS, GC.INT_FIXUP_CAP) >= 3
    refs = R.encode_frames(batch["distinct"], g, batch["scale"])
    assert R.encode_frames(frames, g, batch["scale"])[4] is not refs[0]            # (another call: another memo) ...
    again = R.encode_frames(frames, g, batch["scale"])
    assert all(again[b] is again[b % 4] for b in range(B))                         # ... and one dict per distinct frame inside a call
    queued = []
    for f, e, fast in zip(batch["distinct"], refs, batch["aimed_fast"]):
        assert np.array_equal(R.owners_closed(e["d"], e["pix"], e["ri"]), e["own"])               # owners_loop == owners_closed
        assert np.unique(f[:, 3]).shape[0] == f.shape[0]                                          # intensities that all differ
        q = (e["pix"] < 0) | (e["pix"] % g.W == 0) | (e["d"] == 0)
        assert not (q & fast).any() and np.all((e["d"][fast] >= 0.99) & (e["d"][fast] <= 60.01))
        queued.append(q)
    seam, plain, zero = batch["distinct"][:3]
    assert queued[0][: IC.PAST_HEAD].all() and set((refs[0]["pix"][: IC.PAST_HEAD] // g.W).tolist()) == set(range(g.H)) and not queued[1].any()
    assert 0.70 < queued[0][IC.PAST_HEAD:].mean() < 0.80
    # equal depths inside one pixel: the owner of most seam pixels has later rows of its own depth bits
    e = refs[0]
    tied = [p for p in np.flatnonzero(e["own"] >= 0) if p % g.W == 0 and ((e["pix"] == p) & (e["d"].view(np.uint32) == e["ri"][p].view(np.uint32))).sum() > 1]
    assert len(tied) >= g.H // 2
    # the zero frame: a zero beyond row 300 with 300 seam rows of its own pixel behind it, and an owner that the rule about zeros changes
    e, p0 = refs[2], IC.past_zero_pixel(g)
    z = IC.PAST_ZERO_AT
    assert z > 300 and e["d"][z] == 0 and e["pix"][z] == p0 and np.all(e["pix"][z + 1: z + 1 + 300] == p0) and np.all(e["d"][z + 1: z + 1 + 300] > 0)
    assert int((e["d"] == 0).sum()) == 13 and np.all(e["pix"][e["d"] == 0] == p0)
    no_zero = np.where(e["d"] == 0, -1, e["pix"])
    _, own_without = R.owners_loop(e["d"], no_zero, P)
    assert e["own"][p0] >= 0 and own_without[p0] >= 0 and e["own"][p0] != own_without[p0]
    assert zero[e["own"][p0], :3].tobytes() == zero[own_without[p0], :3].tobytes()                # equal depths before and after the zeros
    assert R.quantise(zero[e["own"][p0], 3:], 255)[0] != R.quantise(zero[own_without[p0], 3:], 255)[0]
    # the two passes' queues
    q_all = np.concatenate([queued[k] for k in which])
    maybe_all = np.concatenate([~batch["aimed_fast"][k] for k in which])
    flagged = np.repeat(np.array([bool((r["d"] == 0).any()) for r in refs])[which], np.diff(offs))
    starts = offs[:-1][which == 2]
    assert (starts > GC.INT_FIXUP_CAP * GC.INT_THREADS).any() and (starts > 2 * GC.INT_FIXUP_CAP * GC.INT_THREADS).any()
    for name, cap, part in (("owner", GC.INT_OWNER_CAP, np.ones(total, bool)), ("fix-up", GC.INT_FIXUP_CAP, flagged)):
        facts = GC.queue_facts(q_all & part, maybe_all & part, total, GC.INT_THREADS, cap, GC.INT_THREADS)
        print("intensity past the grid, %s pass: grid %d, trips %d; chunks that are one drain %d, drains with a remainder %d, refills %d, tails %d"
              % (name, facts["grid"], facts["trips"], facts["full"].size, facts["remainder"].size, facts["refilled"].size, facts["tail"].size))
        assert facts["grid"] == cap
        assert facts["full"].size >= 1 and facts["remainder"].size >= 1 and facts["refilled"].size >= 1, name
        w = int(facts["remainder"][0])
        (a0, a1), (b0, b1) = GC.owner_rows(total, w, 0, cap), GC.owner_rows(total, w, 1, cap)
        assert a1 - a0 == GC.INT_THREADS and b0 == a0 + cap * GC.INT_THREADS and b1 > b0
        assert 1 <= int((q_all & part)[a0:a1].sum()) < GC.INT_THREADS and int((q_all & part)[a0:a1].sum() + (q_all & part)[b0:b1].sum()) > GC.INT_THREADS


def test_quantiser_table():
    w = np.array([np.nan, np.inf, -np.inf, -0.0, -3.0, 1e30, 0.0, 1.0, 0.5, 1.002, 255.4 / 255, 255.6 / 255], np.float32)
    assert R.quantise(w, 255).tolist() == [0, 255, 0, 0, 0, 255, 0, 255, 128, 255, 255, 255]
    assert R.quantise(np.array([0.25, 0.75, 1.25, 1.75, 127.25, 127.75], np.float32), 2).tolist() == [0, 2, 2, 4, 254, 255]   # half to even, clamp
    k = np.arange(100)
    cents = (k / 100).astype(np.float32)
    assert R.quantise(cents, 100).tolist() == k.tolist()
    assert np.array_equal(R.dequantise(R.quantise(cents, 100), 100).view(np.uint32), cents.view(np.uint32))    # bit-exact at scale 100
    w = np.random.default_rng(0).uniform(0, 1, 1000).astype(np.float32)
    assert np.abs(R.dequantise(R.quantise(w, 255), 255).astype(np.float64) - w).max() <= 0.5 / 255 + 2 ** -24
    rounding = IC.rounding()
    e = R.encode_frame(rounding[0]["frames"][0], rounding[0]["g"], 2)
    assert sorted(e["q"].tolist()) == [0, 2, 2]
    e = R.encode_frame(rounding[1]["frames"][0], rounding[1]["g"], 100)
    assert sorted(e["q"].tolist()) == list(range(100))


def test_example_fixture():
    z = np.load(os.path.join(HERE, "golden", "intensity_example_64E.npz"))
    assert z["k"].dtype == np.uint8 and z["k"].shape == (122320,) and z["k"].max() <= 99
    assert os.path.getsize(os.path.join(HERE, "golden", "intensity_example_64E.npz")) < 391924        # below the existing goldens
    b = IC.example()[0]
    e = R.encode_frame(b["frames"][0], b["g"], 100)
    assert np.array_equal(e["payload"], z["payload"]) and e["q"].shape[0] == 94053
    set_ = e["ri"] != 0
    assert np.array_equal(R.dequantise(e["q"], 100).view(np.uint32), b["frames"][0][e["own"][set_], 3].view(np.uint32))


# ---- payload, trailer, container -------------------------------------------------------------------------------------------------
def _payload(n=5, scale=255.0):
    return b"RPI1" + struct.pack("<f", scale) + bytes(range(n))


@pytest.mark.parametrize("parse", ("ref", "product"))
def test_payload_parsing_and_refusals(parse):
    import rpcc_amd  # noqa: F401
    from rpcc_amd import compress_utils as cu
    fn = R.parse_payload if parse == "ref" else cu.parse_intensity_payload
    scale, q = fn(_payload(5, 100.0), 5)
    assert scale == np.float32(100) and q.tolist() == [0, 1, 2, 3, 4]
    assert fn(_payload(0), 0)[1].size == 0
    for bad, n in ((b"RPI2" + _payload()[4:], 5), (_payload()[:7], 0), (b"", 0), (_payload(5, 0.0), 5), (_payload(5, -1.0), 5),
                   (_payload(5, float("nan")), 5), (_payload(5, float("inf")), 5), (_payload(5), 4), (_payload(5), 6)):
        with pytest.raises(ValueError):
            fn(bad, n)
    assert bytes(cu.intensity_payload(np.arange(5), 100.0)) == _payload(5, 100.0)


def _frame_dict(rng, uniform, n=40):
    od = {"residual_quantized": rng.integers(-50, 50, n).astype(np.int16), "contour_map": rng.integers(0, 255, 25).astype(np.uint8),
          "idx_sequence": rng.integers(0, 9, 12).astype(np.uint16), "plane_param": rng.normal(size=(9, 4)).astype(np.float32)}
    if not uniform:
        od["salience_level"] = rng.integers(0, 4, 9).astype(np.uint8)
    return od


@pytest.mark.parametrize("uniform", (True, False))
def test_container_with_trailer(uniform):
    import rpcc_amd  # noqa: F401
    from rpcc_amd import compress_utils as cu
    from rpcc_amd.pipeline import container_spans
    bc = cu.BasicCompressor(method_name="bzip2")
    rng = np.random.default_rng(3)
    od = _frame_dict(rng, uniform)
    plain = cu.pack_bitstream(bc.compress_dict(od), uniform)
    pay = cu.intensity_payload(rng.integers(0, 100, 40), 100.0)
    with_w = cu.pack_bitstream(bc.compress_dict(dict(od, intensity=pay)), uniform)
    coded = bc.compress(pay)
    assert with_w == plain + struct.pack("i", len(coded)) + coded                      # the container without it, plus the trailer
    assert cu.unpack_bitstream(with_w, uniform) == cu.unpack_bitstream(plain, uniform)  # today's dictionary
    assert container_spans(with_w, uniform) == container_spans(plain, uniform)
    span = cu.intensity_trailer_span(with_w, uniform)
    assert span == (len(plain) + 4, len(with_w)) and bc.decompress(with_w[span[0]: span[1]]) == bytes(pay)
    d = cu.unpack_bitstream(with_w, uniform, intensity=True)
    assert d["intensity"] == coded and list(d)[-1] == "intensity"
    # a caller that asks: exactly one length-prefixed payload that ends the blob, else refused
    assert cu.intensity_trailer_span(plain, uniform) is None
    for bad in (plain, with_w + b"\0", with_w[:-1], plain + b"\1\0\0", plain + struct.pack("i", -1), with_w + struct.pack("i", 0), plain[:10]):
        assert cu.intensity_trailer_span(bad, uniform) is None
        with pytest.raises(ValueError):
            cu.unpack_bitstream(bad, uniform, intensity=True)
    assert cu.intensity_trailer_span(plain + struct.pack("i", 0), uniform) == (len(plain) + 4, len(plain) + 4)


@pytest.mark.parametrize("uniform", (True, False))
def test_pack_frames_branches_agree(uniform, monkeypatch):
    """The host-library branch (one call with na + 1 arrays per frame) and the Python branch give the same containers, with and without the
    trailer, and a chunk that mixes both kinds of frames is packed frame by frame."""
    import rpcc_amd  # noqa: F401
    from rpcc_amd import _lib
    from rpcc_amd import compress_utils as cu
    bc = cu.BasicCompressor(method_name="bzip2")
    rng = np.random.default_rng(4)
    frames = [dict(_frame_dict(rng, uniform, n), intensity=cu.intensity_payload(rng.integers(0, 100, n), 255.0)) for n in (0, 7, 300)]
    bare = [{k: v for k, v in od.items() if k != "intensity"} for od in frames]
    want = [cu.pack_bitstream(bc.compress_dict(od), uniform) for od in frames]
    try:
        _lib.host_lib()
        have_host = True
    except _lib.RpccError:
        have_host = False
    if have_host:
        assert cu.pack_frames(bc, frames, uniform) == want
        assert cu.pack_frames(bc, [frames[0], bare[1], frames[2]], uniform) == [want[0], cu.pack_bitstream(bc.compress_dict(bare[1]), uniform), want[2]]
    monkeypatch.setattr(_lib, "host_lib", lambda: (_ for _ in ()).throw(_lib.RpccError("no host library")))
    assert cu.pack_frames(bc, frames, uniform) == want
    assert cu.pack_frames(bc, bare, uniform) == [cu.pack_bitstream(bc.compress_dict(od), uniform) for od in bare]
    for blob, od in zip(want, frames):
        d = cu.unpack_bitstream(blob, uniform, intensity=True)
        assert bc.decompress(d["intensity"]) == bytes(od["intensity"])


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_symbols_version_header_and_bindings(built):
    lib = ctypes.CDLL(built.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "rpcc_hip.h")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in built.exported_symbols()
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    assert built.lib().rpcc_version() == built.ABI_VERSION == 105 and "#define RPCC_ABI_VERSION 105" in hdr
    assert int(re.search(r"#define RPCC_STREAM_E_INTENSITY (\d+)", hdr).group(1)) == built.STREAM_E_INTENSITY == 10
    assert '#include "intensity_kernels.h"' in open(os.path.join(ROOT, "r-pcc_amd", "csrc", "rpcc_hip.hip")).read()


def test_scratch_size(built):
    lib = built.lib()
    for B, P in ((1, 64), (3, 31 * 997), (256, 64 * 2000), (65535, 16)):
        n = lib.rpcc_intensity_scratch_bytes(B, P)
        assert n % 256 == 0 and 8 * B * P <= n <= 8 * B * P + 4 * (B + 1) + 768, (B, P, n)
    for B, P in ((0, 64), (65536, 64), (1, 0), (-1, 64), (1, -5)):
        assert lib.rpcc_intensity_scratch_bytes(B, P) == 0


def test_argument_errors_before_the_device(built):
    """Every pointer is a host dummy that must never reach a kernel: the calls return RPCC_ERR_ARG first."""
    lib = built.lib()
    dummy = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(dummy) + 255) & ~255
    geom = built.Geom(4, 16, 6.2831855, 0.03, -0.43)
    P = 64
    big = 1 << 30

    def enc(rows=p, offs=p, total=10, B=1, g=geom, ri=p, scale=255.0, payload=p, stride=8 + P, nbytes=p, image=None, own=None, orphans=p, scratch=p,
            sbytes=big):
        return lib.rpcc_intensity_encode(rows, offs, total, B, g, ri, scale, payload, stride, nbytes, image, own, orphans, scratch, sbytes, None)

    need = lib.rpcc_intensity_scratch_bytes(1, P)
    for kw in (dict(rows=None), dict(offs=None), dict(ri=None), dict(payload=None), dict(nbytes=None), dict(orphans=None), dict(scratch=None),
               dict(rows=p + 4), dict(rows=p + 8), dict(total=-1), dict(total=1 << 31), dict(B=0), dict(B=65536),
               dict(g=built.Geom(1, 16, 6.28, 0.0, -0.4)), dict(g=built.Geom(0, 16, 6.28, 0.0, -0.4)), dict(g=built.Geom(4, 0, 6.28, 0.0, -0.4)),
               dict(g=built.Geom(128, 1 << 24, 6.28, 0.0, -0.4)), dict(g=built.Geom(4, 16, 0.0, 0.0, -0.4)), dict(g=built.Geom(4, 16, -6.28, 0.0, -0.4)),
               dict(g=built.Geom(4, 16, float("nan"), 0.0, -0.4)),
               dict(scale=0.0), dict(scale=-1.0), dict(scale=float("nan")), dict(scale=float("inf")),
               dict(sbytes=need - 1), dict(sbytes=0), dict(stride=8 + P - 1), dict(stride=0), dict(stride=-5)):
        assert enc(**kw) == -1 and b"bad argument" in lib.rpcc_last_error(), kw

    def dec(payload=p, stride=8 + P, nbytes=p, labels=p, lb=1, B=1, P_=P, out=p, status=p):
        return lib.rpcc_intensity_decode(payload, stride, nbytes, labels, lb, B, P_, out, status, None)

    for kw in (dict(payload=None), dict(nbytes=None), dict(labels=None), dict(out=None), dict(status=None), dict(lb=0), dict(lb=3), dict(lb=4),
               dict(B=0), dict(B=65536), dict(P_=0), dict(stride=8 + P - 1)):
        assert dec(**kw) == -1 and b"bad argument" in lib.rpcc_last_error(), kw


# ---- front-ends -------------------------------------------------------------------------------------------------------------------------
def test_parsers_take_the_flags():
    import rpcc_amd  # noqa: F401
    from rpcc_amd.tools.compress import make_parser
    for datalist in (False, True):
        a = make_parser(datalist=datalist).parse_args([])
        assert a.intensity is False and a.intensity_scale == 255.0
        a = make_parser(datalist=datalist).parse_args(["--intensity", "--intensity_scale", "100"])
        assert a.intensity is True and a.intensity_scale == 100.0


def test_front_ends_that_refuse_intensity(built, tmp_path):
    import torch
    from rpcc_amd import ops
    from rpcc_amd.loader import StreamingCompressor
    from rpcc_amd.pipeline import BatchCompressor, MixedBatchCompressor
    from rpcc_amd.transformer import PCTransformer
    cfg = os.path.join(ROOT, "r-pcc_amd", "lidar_cfg")
    yaml_, csv_ = os.path.join(cfg, "Velodyne_HDL_64E.yaml"), os.path.join(cfg, "Velodyne_HDL_64E_beams.csv")
    T, E = PCTransformer(yaml_, csv_, device="cpu"), PCTransformer(yaml_, device="cpu")
    with pytest.raises(NotImplementedError, match="per-beam elevation table.*last point wins"):
        BatchCompressor(T, intensity_scale=255)
    with pytest.raises(NotImplementedError, match="MixedBatchCompressor: intensity_scale"):
        MixedBatchCompressor({"a": E}, intensity_scale=255)
    bc = BatchCompressor(E, intensity_scale=100)
    assert bc.intensity_scale == 100.0 and BatchCompressor(E).intensity_scale is None
    with pytest.raises(ValueError, match='ingest="rows"'):
        StreamingCompressor(bc, batch=2, ingest="xyz")
    for bad in (0, -1.0, float("nan"), float("inf"), 1e39):
        with pytest.raises(ValueError, match="intensity scale"):
            BatchCompressor(E, intensity_scale=bad)
    with pytest.raises(ValueError, match="no intensity column"):
        ops.intensity_encode(torch.zeros((5, 3)), torch.tensor([0, 5]), E.geom, torch.zeros((1, 64, 2000)), 255.0)
    with pytest.raises(ValueError, match=r"\[N,>=4\] rows"):
        bc._upload([np.zeros((5, 3), np.float32)])


def test_load_rows_and_save_with_intensity(tmp_path):
    import rpcc_amd  # noqa: F401
    from rpcc_amd.dataset import DatasetTemplate as D
    rows = np.random.default_rng(0).normal(size=(7, 4)).astype(np.float32)
    rows[2, :3] = 0                                                           # dropped by the sum != 0 filter, with its intensity
    rows.tofile(tmp_path / "a.bin")
    np.save(tmp_path / "a.npy", rows.astype(np.float64))
    np.savetxt(tmp_path / "a.txt", rows)
    for ext in ("bin", "npy", "txt"):
        got = D.load_rows(str(tmp_path / ("a." + ext)))
        assert got.dtype == np.float32 and got.shape == (7, 4) and np.allclose(got, rows, atol=0 if ext != "txt" else 1e-6)
        assert np.array_equal(D.load_data(str(tmp_path / ("a." + ext)))[:, :3].astype(np.float32), got[:, :3]) or ext == "txt"
    np.save(tmp_path / "b.npy", rows[:, :3])
    with pytest.raises(ValueError, match="no intensity column"):
        D.load_rows(str(tmp_path / "b.npy"))
    keep = np.array([0, 1, 3, 4, 5, 6])
    D.save_point_cloud_to_file(str(tmp_path / "o.bin"), rows[:, :3], intensity=rows[:, 3])
    assert np.array_equal(np.fromfile(tmp_path / "o.bin", np.float32).reshape(-1, 4), rows[keep])
    D.save_point_cloud_to_file(str(tmp_path / "z.bin"), rows[:, :3])
    assert np.array_equal(np.fromfile(tmp_path / "z.bin", np.float32).reshape(-1, 4), np.concatenate([rows[keep, :3], np.zeros((6, 1), np.float32)], 1))
    D.save_point_cloud_to_file(str(tmp_path / "o.npy"), rows[:, :3], intensity=rows[:, 3])
    assert np.array_equal(np.load(tmp_path / "o.npy"), rows[keep])
    D.save_point_cloud_to_file(str(tmp_path / "o.ply"), rows[:, :3], intensity=rows[:, 3])
    raw = open(tmp_path / "o.ply", "rb").read()
    head, body = raw.split(b"end_header\n")
    assert b"property float z\nproperty float intensity\n" in head and b"element vertex 6\n" in head
    assert np.array_equal(np.frombuffer(body, "<f4").reshape(-1, 4), rows[keep])
    D.save_point_cloud_to_file(str(tmp_path / "p.ply"), rows[:, :3])
    assert b"intensity" not in open(tmp_path / "p.ply", "rb").read() and len(open(tmp_path / "p.ply", "rb").read().split(b"end_header\n")[1]) == 72
