"""No GPU: the subpixel specification (tests/subpixel_ref.py) against itself on the example sweep and on the hostile table of
tests/subpixel_cases.py, the derived direction bound, the payload and its refusals, the container with every combination of the two
trailers, the golden containers' bytes without the option, the C ABI's new exports and their argument refusals, and the front ends that refuse the option by name."""
import ctypes
import os
import struct
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import subpixel_cases as SC  # noqa: E402
import subpixel_ref as S  # noqa: E402

BITS = (1, 2, 3, 4)
_MEMO = {}


def case(name):
    if name not in _MEMO:
        _MEMO[name] = (SC.CASES[name](), {})
    return _MEMO[name]


def refs(name, bits):
    batch, memo = case(name)
    return batch, S.encode_frames(batch["frames"], batch["g"], bits, memo)


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    import rpcc_amd  # noqa: F401
    from rpcc_amd import _lib
    return _lib


# ---- the reference against itself ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("small", "round2", "example"))
def test_encode_then_decode_within_half_a_bin(name):
    """Every owner whose row was not clamped comes back within half a code bin on each axis.  With the point's own range r the 3-D error is
    at most r * sqrt((cos(el) * hfov / W)^2 + (vfov / (H-1))^2) / (2 L) (subpixel_ref.direction_bound: two arcs of half a bin, at right
    angles), plus the fp32 roundings the bound does not model: the azimuth is an fp32 value up to 2 pi, so each of its five roundings
    (atan2f within an ulp = two half-ulps, the + 2 pi, the division, the product) moves the direction by at most 2 pi * 2^-24 rad, the
    elevation's four by less, and the three fp32 coordinates of the result by half an ulp of r each: below 24 * 2^-23 * r together."""
    for bits in BITS:
        batch, es = refs(name, bits)
        g = batch["g"]
        tab = S.tables(g)
        for b, (f, e) in enumerate(zip(batch["frames"], es)):
            set_ = e["ri"] != 0
            n = int(set_.sum())
            assert e["payload"].shape[0] == 8 + 2 * n and bytes(e["payload"][:8]) == b"RPS1" + bytes([bits, 0, 0, 0])
            assert int(e["codes"].max(initial=0)) < 1 << bits and not e["codes"][~set_].any()
            pts = S.decode_frame(e["payload"], np.where(set_, 0, 1), e["ri"], g, tab)
            assert pts.dtype == np.float32 and not pts[~set_].view(np.uint32).any()                     # +0.0 where empty
            if n == 0:
                continue
            own = f[e["own"][set_], :3].astype(np.float64)
            err = np.linalg.norm(pts[set_].astype(np.float64) - own, axis=1)
            p = np.flatnonzero(set_)
            r = e["ri"][set_].astype(np.float64)
            bound = r * S.direction_bound(g, bits, g.vertical_FOV * ((p // g.W) / (g.H - 1)) + g.vertical_min) + 24 * 2.0 ** -23 * r
            keep = ~e["clamped"]
            print(name, "bits", bits, "frame", b, "n", n, "clamped", int(e["clamped"].sum()), "max err / bound", float((err[keep] / bound[keep]).max()))
            assert np.all(err[keep] <= bound[keep]), (name, bits, b, float((err[keep] / bound[keep]).max()))
            # on each axis: the offset a code stands for is within half a bin of the offset it codes
            L = 1 << bits
            for off, c in ((e["off_az"], e["az"]), (e["off_el"][keep], e["el"][keep])):
                assert np.all(np.abs(S.step(c.astype(np.float64), bits) - off.astype(np.float64)) <= 0.5 / L + 2.0 ** -24)


def test_example_numbers():
    """What the README says about the example sweep: 94 053 non-empty pixels, 0.9 % of them with a clamped row, and the lateral rms of the
    unclamped rows halving with every bit from 1.46 cm."""
    for bits, want in zip(BITS, (1.46, 0.73, 0.37, 0.18)):
        batch, es = refs("example", bits)
        e, f, g = es[0], batch["frames"][0], batch["g"]
        set_ = e["ri"] != 0
        pts = S.decode_frame(e["payload"], np.where(set_, 0, 1), e["ri"], g)
        err = np.linalg.norm(pts[set_].astype(np.float64) - f[e["own"][set_], :3], axis=1)[~e["clamped"]]
        assert int(set_.sum()) == 94053 and 0.008 < e["clamped"].mean() < 0.011
        assert abs(100 * np.sqrt((err ** 2).mean()) - want) < 0.01, (bits, 100 * np.sqrt((err ** 2).mean()))


@pytest.mark.parametrize("name", ("small", "round2"))
def test_hostile_table_holds_what_it_names(name):
    batch, es = refs(name, 4)
    g, h, e = batch["g"], batch["hostile"], es[0]
    f0 = batch["frames"][0]
    W = g.W
    row, col, off_az, off_el, clamped = S.offsets(f0[: h["n"], :3], g)
    pix = row * W + col
    # every (axis, k) was found, owns its pixel, and its offset is exactly k / 16 - 0.5: t is integral for every bits with L | k ... 16
    assert set(h["exact"]) == {(a, k) for a in ("az", "el") for k in range(SC.STEPS)}
    for (axis, k), i in h["exact"].items():
        off = (off_az if axis == "az" else off_el)[i]
        assert off == np.float32(k / SC.STEPS - 0.5) and not clamped[i] and e["own"][pix[i]] == i, (axis, k)
        for bits in BITS:
            L = 1 << bits
            t = (off + np.float32(0.5)) * np.float32(L)
            c = refs(name, bits)[1][0]["codes"][pix[i], 0 if axis == "az" else 1]
            if (k * L) % SC.STEPS == 0:
                assert t == np.floor(t) and c == k * L // SC.STEPS, (axis, k, bits)        # exactly on a boundary: the upper bin
            else:
                assert c == k * L // SC.STEPS
    top, bottom = h["clamp_top"], h["clamp_bottom"]
    assert off_el[top] == np.float32(0.5) and clamped[top] and row[top] == g.H - 1 and e["codes"][pix[top], 1] == 15
    assert -1 < off_el[bottom] < np.float32(-0.5) and clamped[bottom] and row[bottom] == 0 and e["codes"][pix[bottom], 1] == 0
    assert col[h["wrap"]] == 0 and off_az[h["wrap"]] < 0 and e["own"][pix[h["wrap"]]] == h["wrap"]
    assert off_el[h["far_above"]] > 1 and e["codes"][pix[h["far_above"]], 1] == 15 and off_el[h["far_below"]] < -1 and e["codes"][pix[h["far_below"]], 1] == 0
    i, j = h["tie"]
    assert pix[i] == pix[j] and e["d"][i].view(np.uint32) == e["d"][j].view(np.uint32) and off_az[i] != off_az[j]
    assert e["own"][pix[i]] == i and e["codes"][pix[i], 0] == S.code(off_az[i], 4) != S.code(off_az[j], 4)
    # frame 2 holds the pair in the other order: the other row owns, with the other code
    e2, f2 = es[2], batch["frames"][2]
    o2 = e2["own"][pix[i]]
    assert np.array_equal(f2[o2, :3], f0[j, :3]) and e2["codes"][pix[i], 0] == S.code(off_az[j], 4)
    # the depth-0 scenes: a real row behind the zero owns frame 0's zero pixel (not the nearer one before it); frame 2's is empty
    import intensity_cases as IC
    z = IC.past_zero_pixel(g)
    assert e["ri"][z] == np.float32(e["d"][e["own"][z]]) and e["own"][z] == f0.shape[0] - 1 and e["d"][:e["own"][z]][e["pix"][:e["own"][z]] == z].min() == 0
    assert e2["ri"][z] == 0 and e2["own"][z] == -1 and (e2["pix"] == z).sum() >= 2
    assert (e2["pix"] < 0).sum() == 7                                                  # the NaN / inf rows are skipped
    assert es[1]["payload"].shape[0] == 8                                              # the empty frame: the header alone


def test_past_the_grid_reaches_a_second_trip():
    import subpixel_grid_caps as GC
    batch = case("past_the_grid")[0]
    P = batch["g"].H * batch["g"].W
    B = len(batch["frames"])
    assert GC.code_trips(B * P) == 2 and GC.code_trips((B - 1) * P) == 1
    assert GC.INT_FRAME_PIXELS == 4096 and SC.ROUND2["H"] * SC.ROUND2["W"] == 5000     # round2: a second round of the per-frame kernels, 904 pixels


# ---- payload ---------------------------------------------------------------------------------------------------------------------------
def _payload(n=5, bits=2):
    return b"RPS1" + bytes([bits, 0, 0, 0]) + bytes(i % (1 << bits) for i in range(n)) + bytes((i + 1) % (1 << bits) for i in range(n))


@pytest.mark.parametrize("parse", ("ref", "product"))
def test_payload_parsing_and_refusals(parse):
    import rpcc_amd  # noqa: F401
    from rpcc_amd import compress_utils as cu
    fn = S.parse_payload if parse == "ref" else cu.parse_subpixel_payload
    bits, az, el = fn(_payload(5, 2), 5)
    assert bits == 2 and az.tolist() == [0, 1, 2, 3, 0] and el.tolist() == [1, 2, 3, 0, 1]
    assert fn(_payload(0), 0)[1].size == 0
    good = _payload()
    for bad, n in ((b"RPS2" + good[4:], 5), (b"RPI1" + good[4:], 5), (good[:7], 0), (b"", 0), (good[:4] + b"\0" + good[5:], 5), (good[:4] + b"\5" + good[5:], 5),
                   (good[:5] + b"\1" + good[6:], 5), (good[:6] + b"\1" + good[7:], 5), (good[:7] + b"\1" + good[8:], 5), (good, 4), (good, 6), (good[:-1], 5),
                   (good[:-1] + b"\4", 5), (good[:8] + b"\x10" + good[9:], 5), (_payload(5, 1)[:12] + b"\2" + _payload(5, 1)[13:], 5)):
        with pytest.raises(ValueError):
            fn(bad, n)
    assert bytes(cu.subpixel_payload([0, 1, 2, 3, 0], [1, 2, 3, 0, 1], 2)) == good == bytes(S.payload([0, 1, 2, 3, 0], [1, 2, 3, 0, 1], 2))
    for bad in (0, 5, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="subpixel bits"):
            __import__("rpcc_amd.ops", fromlist=["ops"]).check_subpixel_bits(bad)


def test_tables_are_the_transformers(built):
    from rpcc_amd import ops
    from rpcc_amd.transformer import PCTransformer
    from oracle import oracle as orc
    for name, yaml_ in (("Velodyne64E", "Velodyne_HDL_64E.yaml"),):
        T = PCTransformer(os.path.join(ROOT, "r-pcc_amd", "lidar_cfg", yaml_), device="cpu")
        g = orc.LidarGeom(**orc.GEOMS[name])
        want = S.tables(g)
        got = ops.subpixel_tables(T.H, T.W, T.horizontal_FOV, T.vertical_max, T.vertical_min)
        assert got.dtype == np.float64 and got.tobytes() == want.tobytes() and got.shape[0] == 2 * g.H + 2 * g.W + 256
        # the centre of a cell is no code, but the table's factors are the transform map's: ca * cz, ca * sz, sa rounded to fp32
        H, W = g.H, g.W
        tm = np.stack([got[:H, None] * got[None, 2 * H: 2 * H + W], got[:H, None] * got[None, 2 * H + W: 2 * H + 2 * W], np.repeat(got[H: 2 * H, None], W, 1)], -1)
        assert np.array_equal(tm.astype(np.float32), T.transform_map)


# ---- container -------------------------------------------------------------------------------------------------------------------------
def _frame_dict(rng, uniform, n=40):
    od = {"residual_quantized": rng.integers(-50, 50, n).astype(np.int16), "contour_map": rng.integers(0, 255, 25).astype(np.uint8),
          "idx_sequence": rng.integers(0, 9, 12).astype(np.uint16), "plane_param": rng.normal(size=(9, 4)).astype(np.float32)}
    if not uniform:
        od["salience_level"] = rng.integers(0, 4, 9).astype(np.uint8)
    return od


TRAILERS = ((False, False), (True, False), (False, True), (True, True))


@pytest.mark.parametrize("has", TRAILERS, ids=lambda t: "+".join(n for n, on in zip(("intensity", "subpixel"), t) if on) or "plain")
@pytest.mark.parametrize("uniform", (True, False), ids=("uniform", "nonuniform"))
def test_container_round_trip_and_truncations(uniform, has):
    import rpcc_amd  # noqa: F401
    from rpcc_amd import compress_utils as cu
    bc = cu.BasicCompressor(method_name="bzip2")
    rng = np.random.default_rng(3)
    od = _frame_dict(rng, uniform)
    plain = cu.pack_bitstream(bc.compress_dict(od), uniform)
    if has[0]:
        od["intensity"] = cu.intensity_payload(rng.integers(0, 256, 40), 100.0)
    if has[1]:
        od["subpixel"] = cu.subpixel_payload(rng.integers(0, 4, 40), rng.integers(0, 4, 40), 2)
    names = tuple(n for n, on in zip(("intensity", "subpixel"), has) if on)
    assert cu._keys(uniform, od) == tuple(c.name for c in cu.columns(uniform, *has)) and cu._keys(uniform, od)[len(cu.columns(uniform)):] == names
    coded = bc.compress_dict({k: od[k] for k in cu._keys(uniform, od)})
    blob = cu.pack_bitstream(coded, uniform)
    assert blob[: len(plain)] == plain                                              # without the options: the same bytes, and a prefix with them
    assert blob == plain + b"".join(struct.pack("i", len(coded[n])) + coded[n] for n in names)
    assert cu.pack_frames(bc, [od, od], uniform) == [blob, blob]                    # the chunked host packer (or the Python path) with the extra arrays
    assert cu.unpack_bitstream(blob, uniform) == {k: coded[k] for k in cu._keys(uniform)}      # a reader that asks for nothing: as ever
    got = cu.unpack_bitstream(blob, uniform, intensity=has[0], subpixel=has[1])
    assert got == coded and tuple(got) == cu._keys(uniform, od)
    for n in names:
        assert bytes(bc.decompress(got[n])) == od[n].tobytes()
    # every other set of flags is refused, and the text names the flag that does not fit
    for ask in TRAILERS:
        if ask == has or ask == (False, False):
            continue
        if sum(ask) == sum(has):     # one trailer, the other one asked for: the container names no payload, so it reads -- and the payload's magic refuses it
            other = cu.unpack_bitstream(blob, uniform, intensity=ask[0], subpixel=ask[1])
            with pytest.raises(ValueError, match="no b'RP[IS]1' header"):
                (cu.parse_subpixel_payload if ask[1] else cu.parse_intensity_payload)(bc.decompress(other["subpixel" if ask[1] else "intensity"]), 40)
            continue
        with pytest.raises(ValueError) as e:
            cu.unpack_bitstream(blob, uniform, intensity=ask[0], subpixel=ask[1])
        asked = [n for n, on in zip(("intensity", "subpixel"), ask) if on]
        if sum(has) < sum(ask):                                                     # fewer trailers than asked for: the first one missing
            assert "no %s trailer" % asked[sum(has)] in str(e.value), (has, ask, str(e.value))
        elif sum(has) > sum(ask):                                                   # two in the blob, one asked for: the other flag is named
            assert "%s=True" % ({"intensity", "subpixel"} - set(asked)).pop() in str(e.value), (has, ask, str(e.value))
    if names:
        # every truncation of the trailers is refused by the reader that asks for them; a reader that asks for nothing still reads the geometry
        for cut in range(len(plain), len(blob)):
            with pytest.raises(ValueError):
                cu.unpack_bitstream(blob[:cut], uniform, intensity=has[0], subpixel=has[1])
            assert cu.unpack_bitstream(blob[:cut], uniform) == cu.unpack_bitstream(plain, uniform)
        for cut in range(len(plain)):
            with pytest.raises(ValueError):
                cu.unpack_bitstream(blob[:cut], uniform, intensity=has[0], subpixel=has[1])
        with pytest.raises(ValueError, match="must end the container"):
            cu.unpack_bitstream(blob + b"\0", uniform, intensity=has[0], subpixel=has[1])
    if has == (True, False):
        assert cu.intensity_trailer_span(blob, uniform) == (len(plain) + 4, len(blob))


def test_frame_slices_with_the_second_trailer():
    import torch
    import rpcc_amd  # noqa: F401
    from rpcc_amd import compress_utils as cu
    rng = np.random.default_rng(3)
    K, P = 5, 13
    counts = np.array([[4, 0, 9, 0, 0], [13, 0, 0, 0, 0], [1, 0, 2, 0, 10]], np.int32)
    nnz, nseq = np.array([7, 0, 5], np.int32), np.array([3, 0, 4], np.int32)
    nbytes, nsub = np.array([8 + 7, 8, 8 + 5], np.int32), np.array([8 + 14, 8, 8 + 10], np.int32)
    bufs = dict(salience_level=rng.integers(0, 4, (3, K)).astype(np.uint8), contour_map=rng.integers(0, 256, (3, (P + 7) // 8)).astype(np.uint8),
                idx_sequence=rng.integers(0, 9, (3 * P,)).astype(np.uint16), plane_param=rng.standard_normal((3, K, 4)).astype(np.float32),
                residual_quantized=rng.integers(-9, 9, (3 * P,)).astype(np.int16), intensity=rng.integers(0, 256, (3, 8 + P)).astype(np.uint8),
                subpixel=rng.integers(0, 4, (3, 8 + 2 * P)).astype(np.uint8))
    assert [c.name for c in cu.SCHEMA][-2:] == ["intensity", "subpixel"] and cu.SCHEMA[-1].bound(P, K) == 8 + 2 * P and cu.SCHEMA[-1].dtype == np.uint8
    for has in TRAILERS:
        cols = cu.columns(False, *has)
        at = cu.frame_slices(cols, bufs, counts, nnz, nseq, nbytes if has[0] else None, nsub if has[1] else None)
        assert list(at) == [c.name for c in cols]
        if has[1]:
            assert at["subpixel"][0].tolist() == [0, 8 + 2 * P, 2 * (8 + 2 * P)] and at["subpixel"][1].tolist() == nsub.tolist()
            tt = cu.frame_slices(cols, {k: torch.from_numpy(v) for k, v in bufs.items()}, *(None if v is None else torch.from_numpy(v)
                                 for v in (counts, nnz, nseq, nbytes if has[0] else None, nsub)))
            assert tt["subpixel"][0].tolist() == at["subpixel"][0].tolist() and tt["subpixel"][1].tolist() == nsub.tolist()
        payload = cu.BatchPayload(cols, bufs, counts, nnz, nseq, nbytes if has[0] else None, nsub=nsub if has[1] else None)
        for b in range(3):
            od = payload.frame(b)
            assert cu._keys(False, od) == tuple(c.name for c in cols)
            if has[1]:
                assert od["subpixel"].tobytes() == bufs["subpixel"][b, : nsub[b]].tobytes() and np.shares_memory(od["subpixel"], bufs["subpixel"])
            if has[0]:
                assert od["intensity"].tobytes() == bufs["intensity"][b, : nbytes[b]].tobytes()


# ---- C ABI -----------------------------------------------------------------------------------------------------------------------------
def test_abi_exports_and_version(built):
    hdr = open(os.path.join(ROOT, "include", "rpcc_hip.h")).read()
    lib = ctypes.CDLL(built.LIB_PATH)
    for name in ("rpcc_subpixel_scratch_bytes", "rpcc_subpixel_encode", "rpcc_subpixel_decode"):
        assert hasattr(lib, name) and name in built.exported_symbols() and name + "(" in hdr, name
    assert "#define RPCC_STREAM_E_SUBPIXEL 11" in hdr and built.STREAM_E_SUBPIXEL == 11
    assert built.lib().rpcc_version() == built.ABI_VERSION == 105 and "#define RPCC_ABI_VERSION 105" in hdr
    need = built.lib().rpcc_subpixel_scratch_bytes
    for B, P in ((1, 64), (3, 5000), (256, 128000)):
        assert need(B, P) >= built.lib().rpcc_intensity_scratch_bytes(B, P) + 2 * B * P and need(B, P) % 256 == 0
    assert need(0, 64) == 0 and need(1, 0) == 0 and need(65536, 64) == 0
    assert need(1, (1 << 30) - 4) == 0 and need(1, (1 << 30) - 5) > 0 and built.lib().rpcc_intensity_scratch_bytes(1, 1 << 30) > 0     # 8 + 2 P fits an int32


def test_argument_errors_before_the_device(built):
    """Every pointer is a host dummy that must never reach a kernel: the calls return RPCC_ERR_ARG first."""
    lib = built.lib()
    dummy = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(dummy) + 255) & ~255
    geom = built.Geom(4, 16, 6.2831855, 0.03, -0.43)
    P = 64
    big = 1 << 30

    def enc(rows=p, offs=p, total=10, B=1, g=geom, ri=p, bits=2, payload=p, stride=8 + 2 * P, nbytes=p, codes=None, orphans=p, scratch=p, sbytes=big):
        return lib.rpcc_subpixel_encode(rows, offs, total, B, g, ri, bits, payload, stride, nbytes, codes, orphans, scratch, sbytes, None)

    need = lib.rpcc_subpixel_scratch_bytes(1, P)
    for kw in (dict(rows=None), dict(offs=None), dict(ri=None), dict(payload=None), dict(nbytes=None), dict(orphans=None), dict(scratch=None),
               dict(rows=p + 4), dict(rows=p + 8), dict(total=-1), dict(total=1 << 31), dict(B=0), dict(B=65536), dict(codes=p + 1),
               dict(g=built.Geom(1, 16, 6.28, 0.0, -0.4)), dict(g=built.Geom(0, 16, 6.28, 0.0, -0.4)), dict(g=built.Geom(4, 0, 6.28, 0.0, -0.4)),
               dict(g=built.Geom(128, 1 << 24, 6.28, 0.0, -0.4)), dict(g=built.Geom(4, 16, 0.0, 0.0, -0.4)), dict(g=built.Geom(4, 16, -6.28, 0.0, -0.4)),
               dict(g=built.Geom(4, 16, float("nan"), 0.0, -0.4)), dict(g=built.Geom(64, 1 << 24, 6.28, 0.0, -0.4), stride=1 << 40),      # 8 + 2 P past int32
               dict(g=built.Geom(4, (1 << 28) - 1, 6.28, 0.0, -0.4), stride=1 << 40), dict(bits=0), dict(bits=5), dict(bits=-1), dict(bits=8),
               dict(sbytes=need - 1), dict(sbytes=0), dict(stride=8 + 2 * P - 1), dict(stride=8 + P), dict(stride=0), dict(stride=-5)):
        before = bytes(dummy)
        assert enc(**kw) == -1 and b"bad argument" in lib.rpcc_last_error(), kw
        assert bytes(dummy) == before

    def dec(payload=p, stride=8 + 2 * P, nbytes=p, labels=p, lb=1, ri=p, tables=p, H=4, W=16, B=1, out=p, status=p):
        return lib.rpcc_subpixel_decode(payload, stride, nbytes, labels, lb, ri, tables, H, W, B, out, status, None)

    for kw in (dict(payload=None), dict(nbytes=None), dict(labels=None), dict(ri=None), dict(tables=None), dict(out=None), dict(status=None),
               dict(lb=0), dict(lb=3), dict(lb=4), dict(B=0), dict(B=65536), dict(H=1), dict(H=0), dict(W=0), dict(H=128, W=1 << 24), dict(H=64, W=1 << 24, stride=1 << 40), dict(H=4, W=(1 << 28) - 1, stride=1 << 40),
               dict(tables=p + 4),
               dict(stride=8 + 2 * P - 1), dict(stride=8 + P)):
        before = bytes(dummy)
        assert dec(**kw) == -1 and b"bad argument" in lib.rpcc_last_error(), kw
        assert bytes(dummy) == before


# ---- front ends --------------------------------------------------------------------------------------------------------------------------
def test_front_ends_that_refuse_subpixel(built):
    import torch
    from rpcc_amd import compress_utils as cu
    from rpcc_amd import ops
    from rpcc_amd.loader import StreamingCompressor
    from rpcc_amd.pipeline import BatchCompressor, BatchDecompressor, MixedBatchCompressor
    from rpcc_amd.tools import compress as tc
    from rpcc_amd.tools import decompress_datalist as tdd
    from rpcc_amd.transformer import PCTransformer
    cfg = os.path.join(ROOT, "r-pcc_amd", "lidar_cfg")
    yaml_, csv_ = os.path.join(cfg, "Velodyne_HDL_64E.yaml"), os.path.join(cfg, "Velodyne_HDL_64E_beams.csv")
    T, E = PCTransformer(yaml_, csv_, device="cpu"), PCTransformer(yaml_, device="cpu")
    with pytest.raises(NotImplementedError, match="BatchCompressor: subpixel with a per-beam elevation table.*last point wins"):
        BatchCompressor(T, subpixel_bits=2)
    with pytest.raises(NotImplementedError, match="subpixel with a per-beam elevation table"):
        cu.encode_subpixel(T, np.zeros((5, 4), np.float32), np.zeros((64, 2000), np.float32), 2)
    with pytest.raises(NotImplementedError, match="subpixel with a per-beam elevation table"):
        T.subpixel_tables()
    with pytest.raises(NotImplementedError, match="MixedBatchCompressor: subpixel_bits"):
        MixedBatchCompressor({"a": E}, subpixel_bits=2)
    with pytest.raises(NotImplementedError, match="BatchDecompressor: subpixel"):
        BatchDecompressor(E, 100, 0.04, subpixel=True)
    for flag in ("--batch_decode", "--stream_decode"):
        args = tc.make_parser(datalist=True).parse_args(["--datalist", "none.txt", "--output_dir", "none", "--lidar", "Velodyne64E", flag, "--subpixel"])
        with pytest.raises(NotImplementedError, match="--%s with --subpixel" % flag[2:]):
            tdd.decompress(args)
        args.subpixel = 0                                         # any value given turns the option on when decompressing
        with pytest.raises(NotImplementedError, match="--%s with --subpixel" % flag[2:]):
            tdd.decompress(args)
    bc = BatchCompressor(E, subpixel_bits=3)
    assert bc.subpixel_bits == 3 and BatchCompressor(E).subpixel_bits is None and [c.name for c in bc.columns][-1] == "subpixel"
    assert [c.name for c in BatchCompressor(E, subpixel_bits=1, intensity_scale=100).columns][-2:] == ["intensity", "subpixel"]
    with pytest.raises(ValueError, match='ingest="rows"'):
        StreamingCompressor(bc, batch=2, ingest="xyz")
    for bad in (0, 5, 2.5, "2"):
        with pytest.raises(ValueError, match="subpixel bits"):
            BatchCompressor(E, subpixel_bits=bad)
    with pytest.raises(ValueError, match="16-byte rows"):
        ops.subpixel_encode(torch.zeros((5, 3)), torch.tensor([0, 5]), E.geom, torch.zeros((1, 64, 2000)), 2)
    # the tools' flag: BITS when compressing, bare when decompressing
    parse = lambda *a: tc.make_parser().parse_args(["--input", "x.bin", "--output", "y.rpcc", "--lidar", "Velodyne64E"] + list(a))
    assert tc.subpixel_bits_of(parse()) is None and tc.subpixel_bits_of(parse("--subpixel", "3")) == 3 and parse("--subpixel").subpixel == tc.SUBPIXEL_FLAG
    for bad in (("--subpixel",), ("--subpixel", "0"), ("--subpixel", "5")):
        with pytest.raises(ValueError, match="subpixel"):
            tc.subpixel_bits_of(parse(*bad))
    assert cu.rows16(np.ones((3, 3))).tolist() == [[1, 1, 1, 0]] * 3 and cu.rows16(np.ones((2, 5))).shape == (2, 4)


# ---- without the option: the golden containers' bytes -----------------------------------------------------------------------------------
GEOMETRY = ("contour_map", "idx_sequence", "plane_param", "residual_quantized")
GOLDEN_BLOBS = (("example_64E.npz", "rpcc", True), ("pins_example_64E.npz", "rpcc_uniform_plane", True), ("pins_example_64E.npz", "rpcc_nonuniform_plane", False),
                ("pins_synth_vlp16.npz", "rpcc_nonuniform_plane", False))


@pytest.mark.parametrize("file,key,uniform", GOLDEN_BLOBS, ids=["%s:%s" % (f[:-4], k) for f, k, _ in GOLDEN_BLOBS])
def test_golden_containers_come_back_without_the_option(file, key, uniform):
    """The stored .rpcc containers (written by earlier versions of this build, bzip2) taken apart by unpack_bitstream / decompress_dict and
    put together again through every packing path with the default arguments -- no intensity, no subpixel, nsub=None: the golden bytes."""
    import rpcc_amd  # noqa: F401
    from rpcc_amd import compress_utils as cu
    names = GEOMETRY if uniform else ("salience_level",) + GEOMETRY
    assert tuple(c.name for c in cu.columns(uniform)) == names == cu._keys(uniform) and len(names) == (4 if uniform else 5)
    assert tuple(c.name for c in cu.columns(uniform, True)) == names + ("intensity",) == cu._keys(uniform, {"intensity": 0})
    blob = np.load(os.path.join(SC.GOLDEN, file))[key].tobytes()
    bc = cu.BasicCompressor(method_name="bzip2")
    coded = cu.unpack_bitstream(blob, uniform)
    assert tuple(coded) == names and cu.pack_bitstream(coded, uniform) == blob and cu.unpack_bitstream(blob, uniform, intensity=False, subpixel=False) == coded
    for flags in (dict(intensity=True), dict(subpixel=True), dict(intensity=True, subpixel=True)):
        with pytest.raises(ValueError, match="no (intensity|subpixel) trailer"):
            cu.unpack_bitstream(blob, uniform, **flags)
    schema = {c.name: c for c in cu.SCHEMA}
    od = {k: np.frombuffer(v, dtype=schema[k].dtype) for k, v in bc.decompress_dict(coded).items()}
    od["plane_param"] = od["plane_param"].reshape(-1, 4)
    assert cu.pack_bitstream(bc.compress_dict(od), uniform) == blob
    assert cu.pack_frames(bc, [od, od], uniform) == [blob, blob]
    # the same frame cut out of a batch's padded buffers by BatchPayload with the default arguments (two frames: the golden one twice)
    K = od["plane_param"].shape[0]
    pad = lambda a, shape: np.concatenate([a.reshape(-1), np.zeros(int(np.prod(shape)) - a.size, a.dtype)]).reshape(shape)
    bufs = dict(contour_map=np.stack([od["contour_map"]] * 2), plane_param=np.stack([od["plane_param"]] * 2),
                idx_sequence=np.concatenate([od["idx_sequence"]] * 2), residual_quantized=np.concatenate([od["residual_quantized"]] * 2),
                salience_level=None if uniform else np.stack([pad(od["salience_level"], (K,))] * 2))
    counts = np.zeros((2, K), np.int32)
    counts[:, K - 1] = 1                                                            # nrow = K: every stored model row (and salience entry) counts
    assert uniform or od["salience_level"].shape[0] == K
    n_q, n_s = od["residual_quantized"].shape[0], od["idx_sequence"].shape[0]
    payload = cu.BatchPayload(cu.columns(uniform), bufs, counts, np.array([n_q] * 2, np.int32), np.array([n_s] * 2, np.int32))
    frames = [payload.frame(b) for b in range(2)]
    assert all(tuple(sorted(f)) == tuple(sorted(names)) for f in frames)
    assert cu.pack_frames(bc, frames, uniform) == [blob, blob] and [cu.pack_bitstream(bc.compress_dict(f), uniform) for f in frames] == [blob, blob]
