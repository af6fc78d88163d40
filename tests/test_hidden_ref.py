"""No GPU: the hidden_points specification (tests/hidden_ref.py) against itself on the cases of tests/hidden_cases.py, the error bound of
the range code at its ties and at the 65535 edge, the payload and its refusals, the container with every combination of the three
trailers, frame_slices / BatchPayload with the new column, the C ABI's new exports and their argument refusals, and the front ends that
refuse the option by name."""
import ctypes
import itertools
import os
import struct
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import hidden_cases as HC  # noqa: E402
import hidden_ref as R  # noqa: E402
from oracle import oracle as orc  # noqa: E402

_MEMO = {}
NAMES = ("intensity", "subpixel", "hidden_points")


def refs(name, bits):
    if name not in _MEMO:
        _MEMO[name] = (HC.CASES[name](), {})
    batch, memo = _MEMO[name]
    return batch, R.encode_frames(batch["frames"], batch["g"], batch["step"], bits, memo)


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    import rpcc_amd  # noqa: F401
    from rpcc_amd import _lib
    return _lib


# ---- the reference against itself ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("small", "round2", "crowd", "example"))
def test_reference_self_checks(name):
    """Counts sum to m, no pixel carries more than 255, the order is (pixel, key), every input point is the owner of a pixel, skipped,
    carried or counted as uncarried, and decode(encode) gives one point per carried hidden point within the range code's bound."""
    for bits in (0, 2):
        batch, es = refs(name, bits)
        g = batch["g"]
        tm = orc.transform_map(g).reshape(-1, 3)
        for f, e in zip(batch["frames"], es):
            n, m = e["n"], e["m"]
            assert n == int((e["ri"] != 0).sum()) and int(e["counts"].sum(dtype=np.int64)) == m and e["counts"].shape[0] == n
            assert e["payload"].shape[0] == 16 + n + (4 if bits else 2) * m
            assert bytes(e["payload"][:8]) == b"RPH1" + bytes([bits, 0, 0, 0]) and struct.unpack_from("<fI", e["payload"].tobytes(), 8) == (np.float32(batch["step"]), m)
            order = e["pixel"].astype(np.int64) << 32 | e["key"].astype(np.int64)
            assert np.all(np.diff(order) >= 0)
            valid = (e["pix"] >= 0) & (e["d"] != 0)
            owners = int((e["own"] >= 0).sum())
            assert owners == n and int(valid.sum()) == owners + m + e["uncarried"] and int(e["hidden"].sum()) == m + e["uncarried"]
            assert int(e["az"].max(initial=0)) < 1 << bits and int(e["el"].max(initial=0)) < 1 << bits
            pts = R.decode_frame(e["payload"], np.where(e["ri"] != 0, 0, 1), g, tm)
            assert pts.dtype == np.float32 and pts.shape == (m, 3)
            # (carried[j] is the row whose key stands at place j)
            r = R.decoded_range(e["k"], batch["step"])
            d = e["d"][e["carried"]]
            assert np.all(np.abs(r.astype(np.float64) - d.astype(np.float64)) <= R.error_bound(e["k"], batch["step"]))
            if bits == 0:   # on the pixel's centre ray at the decoded range
                assert np.allclose(np.linalg.norm(pts.astype(np.float64), axis=1), r, rtol=1e-6, atol=1e-7)
    if name == "crowd":
        batch, es = refs(name, 0)
        e, g = es[0], batch["g"]
        per_pixel = dict(zip(np.flatnonzero(e["ri"] != 0).tolist(), e["counts"].tolist()))
        for row, col, rows in HC.CROWD_AT:
            assert int((e["pix"] == row * g.W + col).sum()) == rows and per_pixel[row * g.W + col] == min(rows - 1, 255), (row, col)
        assert [per_pixel[r * g.W + c] for r, c, _ in HC.CROWD_AT] == [255, 254, 255, 255] and e["counts"].max() == 255
        assert e["uncarried"] == (3000 - 1 - 255) + (257 - 1 - 255)
    if name == "example":
        batch, es = refs(name, 0)
        assert es[0]["n"] + es[0]["m"] == batch["frames"][0].shape[0] == 122320 and es[0]["uncarried"] == 0 and es[0]["n"] == 94053


def test_the_cap_keeps_the_smallest_keys():
    batch, es = refs("crowd", 2)
    e, f = es[0], batch["frames"][0]
    row, col, rows = HC.CROWD_AT[0]
    p = row * batch["g"].W + col
    mine = np.flatnonzero(e["hidden"] & (e["pix"] == p))
    k, fits = R.range_code(e["d"][mine], batch["step"])
    assert fits.all() and mine.shape[0] >= rows - 1
    kept = e["key"][e["pixel"] == p]
    assert kept.shape[0] == 255
    # every key that was dropped is at least the largest one kept
    import subpixel_ref as SR
    _, _, oa, oe, _ = SR.offsets(f[mine, :3], batch["g"])
    keys = np.sort(k.astype(np.uint32) << 8 | SR.code(oa, 2).astype(np.uint32) << 4 | SR.code(oe, 2).astype(np.uint32))
    assert np.array_equal(keys[:255], kept) and keys[255] >= kept[-1]


def test_error_bound_at_ties_and_edges():
    """A power-of-two step: d / step and k * step are exact, so a range on (k + 0.5) * step is a tie (half to even) and the error is exactly
    half a step; either side of k = 65535."""
    step = np.float32(2.0 ** -5)
    ks = np.array([0, 1, 2, 3, 10, 11, 4095, 4096, 65533, 65534], np.float64)
    d = ((ks + 0.5) * float(step)).astype(np.float32)
    k, fits = R.range_code(d, step)
    assert fits.all() and np.array_equal(k, np.where(ks % 2 == 0, ks, ks + 1).astype(np.float32))          # ties to even
    assert np.array_equal(np.abs(R.decoded_range(k, step).astype(np.float64) - d), np.full(ks.shape, 0.5 * float(step)))
    for kk in (0, 1, 37, 65535):
        k, fits = R.range_code(np.float32(kk * float(step)), step)
        assert fits and k == kk and R.decoded_range(k, step) == np.float32(kk * float(step))
    edge = np.float32(65535.5 * float(step))
    below = np.nextafter(edge, np.float32(0))
    assert R.range_code(below, step) == (np.float32(65535), True)
    assert R.range_code(edge, step)[0] == 65536 and not R.range_code(edge, step)[1]                          # the tie goes to the even 65536: not carried
    assert not R.range_code(np.float32(65536 * float(step)), step)[1] and not R.range_code(np.float32(np.inf), step)[1]
    assert not R.range_code(np.float32(3.0e38), np.float32(1e-3))[1]                                         # the quotient overflows: !(k <= 65535)
    # the bound with a step that is no power of two, on random ranges: |r - d| <= step * (0.5 + k * 2^-23) < step * (0.5 + 2^-7)
    rng = np.random.default_rng(0)
    for s in (np.float32(0.04), np.float32(0.1), np.float32(0.013)):
        d = rng.uniform(0, 65535 * float(s), 200000).astype(np.float32)
        k, fits = R.range_code(d, s)
        k, d = k[fits], d[fits]
        err = np.abs(R.decoded_range(k, s).astype(np.float64) - d.astype(np.float64))
        assert np.all(err <= R.error_bound(k, s)) and np.all(R.error_bound(k, s) < float(s) * (0.5 + 2.0 ** -7))


def test_edge_rows_of_the_cases():
    batch, es = refs("small", 0)
    e, where = es[0], batch["edge"]
    base = batch["frames"][0].shape[0] - len(where)
    carried = set(e["carried"].tolist())
    got = {k: base + i in carried for k, i in where.items()}
    assert got == dict(owner=False, tie_even=True, tie_odd=True, on_code=True, below_tie=True, above_tie=True, same_a=True, same_b=True, same_c=True,
                       last=True, last_tie_below=True, last_tie=False, first_out=False, far_out=False)
    kof = {k: int(e["k"][np.flatnonzero(e["carried"] == base + i)[0]]) for k, i in where.items() if got[k]}
    assert (kof["tie_even"], kof["tie_odd"], kof["on_code"], kof["below_tie"], kof["above_tie"], kof["last"], kof["last_tie_below"]) == (10, 12, 37, 20, 21, 65535, 65535)
    assert kof["same_a"] == kof["same_b"] == kof["same_c"] == 123
    assert e["own"][e["pix"][base + where["owner"]]] == base + where["owner"] and e["uncarried"] >= 3
    # frame 2: a pixel emptied by a last depth-0 row -- its rows are hidden points that are not carried
    e2 = es[2]
    lost = e2["hidden"] & (e2["ri"][np.maximum(e2["pix"], 0)] == 0)
    assert lost.any() and not np.isin(np.flatnonzero(lost), e2["carried"]).any()
    # a hidden point nearer than the owner of its pixel (in front of a depth-0 row) and one of equal depth bits
    e0 = es[0]
    own_d = e0["ri"][e0["pix"][e0["carried"]]]
    assert (e0["d"][e0["carried"]] < own_d).any() and (e0["d"][e0["carried"]].view(np.uint32) == own_d.view(np.uint32)).any()


def test_payload_refusals_in_words(built):
    from rpcc_amd import compress_utils as cu
    batch, es = refs("small", 2)
    e = es[0]
    n, m, raw = e["n"], e["m"], e["payload"].tobytes()
    assert cu.HIDDEN_MAGIC == R.MAGIC
    assert cu.hidden_payload(2, batch["step"], e["counts"], e["k"], e["az"], e["el"]).tobytes() == raw
    got = cu.parse_hidden_payload(raw, n)
    want = R.parse_payload(raw, n)
    assert got[0] == want[0] == 2 and got[1] == want[1] and all(np.array_equal(a, b) for a, b in zip(got[2:], want[2:]))
    e0 = refs("small", 0)[1][0]
    assert cu.hidden_payload(0, batch["step"], e0["counts"], e0["k"]).tobytes() == e0["payload"].tobytes()
    assert cu.parse_hidden_payload(e0["payload"], n)[0] == 0 and not cu.parse_hidden_payload(e0["payload"], n)[4].any()

    def put(at, value):
        b = bytearray(raw)
        b[at: at + len(value)] = value
        return bytes(b)

    bad = {"no b'RPH1' header": [raw[:15], b"", put(3, b"2"), put(2, b"S")], "bits per axis": [put(4, b"\x05"), put(4, b"\xff")],
           "reserved bytes": [put(5, b"\x01"), put(6, b"\x01"), put(7, b"\x01")],
           "step": [put(8, struct.pack("<f", 0.0)), put(8, struct.pack("<f", -1.0)), put(8, struct.pack("<f", np.inf)), put(8, struct.pack("<f", np.nan))],
           "bytes for": [raw + b"\0", raw[:-1], put(12, struct.pack("<I", m + 1)), put(12, struct.pack("<I", 0xFFFFFFFF))],
           "the counts sum to": [put(16, bytes([raw[16] + 1]))], "code 4 at 2 bits": [put(16 + n + 2 * m, b"\x04"), put(len(raw) - 1, b"\x04")]}
    for text, blobs in bad.items():
        for b in blobs:
            with pytest.raises(ValueError, match="hidden_points payload: .*" + text):
                cu.parse_hidden_payload(b, n)
            with pytest.raises(ValueError):
                R.parse_payload(b, n)
    with pytest.raises(ValueError, match="bytes for"):
        cu.parse_hidden_payload(raw, n + 1)
    with pytest.raises(ValueError, match="room for"):
        R.parse_payload(raw, n, capacity=m - 1)
    with pytest.raises(ValueError, match="the counts sum"):
        cu.hidden_payload(0, 0.04, [1, 2], [5])
    for s in (0.0, -1.0, float("nan"), float("inf"), 1e39):
        with pytest.raises(ValueError, match="hidden_points step"):
            cu.hidden_payload(0, s, [], [])
    for b in (-1, 5, 1.5, "2", True):
        with pytest.raises(ValueError, match="hidden_points bits"):
            cu.hidden_payload(b, 0.04, [], [])


# ---- container -------------------------------------------------------------------------------------------------------------------------
def _frame_dict(rng, uniform, n=40):
    od = {"residual_quantized": rng.integers(-50, 50, n).astype(np.int16), "contour_map": rng.integers(0, 255, 25).astype(np.uint8),
          "idx_sequence": rng.integers(0, 9, 12).astype(np.uint16), "plane_param": rng.normal(size=(9, 4)).astype(np.float32)}
    if not uniform:
        od["salience_level"] = rng.integers(0, 4, 9).astype(np.uint8)
    return od


TRAILERS = tuple(itertools.product((False, True), repeat=3))
PARSE = dict(intensity="parse_intensity_payload", subpixel="parse_subpixel_payload", hidden_points="parse_hidden_payload")


@pytest.mark.parametrize("has", TRAILERS, ids=lambda t: "+".join(n for n, on in zip(NAMES, t) if on) or "plain")
@pytest.mark.parametrize("uniform", (True, False), ids=("uniform", "nonuniform"))
def test_container_round_trip_and_truncations(uniform, has):
    import rpcc_amd  # noqa: F401
    from rpcc_amd import compress_utils as cu
    bc = cu.BasicCompressor(method_name="bzip2")
    rng = np.random.default_rng(3)
    od = _frame_dict(rng, uniform)
    plain = cu.pack_bitstream(bc.compress_dict(od), uniform)
    before = {}                                                                          # the blob with the older trailers only: today's bytes
    if has[0]:
        od["intensity"] = cu.intensity_payload(rng.integers(0, 256, 40), 100.0)
    if has[1]:
        od["subpixel"] = cu.subpixel_payload(rng.integers(0, 4, 40), rng.integers(0, 4, 40), 2)
    older = cu.pack_bitstream(bc.compress_dict(od), uniform)
    if has[2]:
        counts = rng.integers(0, 3, 40)
        m = int(counts.sum())
        od["hidden_points"] = cu.hidden_payload(2, 0.04, counts, rng.integers(0, 4000, m), rng.integers(0, 4, m), rng.integers(0, 4, m))
    names = tuple(n for n, on in zip(NAMES, has) if on)
    assert cu.TRAILERS == NAMES
    assert cu._keys(uniform, od) == tuple(c.name for c in cu.columns(uniform, *has)) and cu._keys(uniform, od)[len(cu.columns(uniform)):] == names
    coded = bc.compress_dict({k: od[k] for k in cu._keys(uniform, od)})
    blob = cu.pack_bitstream(coded, uniform)
    assert blob[: len(plain)] == plain and blob[: len(older)] == older                     # without the new trailer: the same bytes, and a prefix with it
    assert (blob == older) == (not has[2])
    assert blob == plain + b"".join(struct.pack("i", len(coded[n])) + coded[n] for n in names)
    assert cu.pack_frames(bc, [od, od], uniform) == [blob, blob]                            # the chunked host packer (or the Python path) with the extra arrays
    assert cu.unpack_bitstream(blob, uniform) == {k: coded[k] for k in cu._keys(uniform)}   # a reader that asks for nothing: as ever
    got = cu.unpack_bitstream(blob, uniform, *has)
    assert got == coded and tuple(got) == cu._keys(uniform, od)
    assert cu.unpack_bitstream(blob, uniform, intensity=has[0], subpixel=has[1], hidden_points=has[2]) == got
    for n in names:
        assert bytes(bc.decompress(got[n])) == od[n].tobytes()
    # every other set of flags is refused, and the text names the flag that does not fit
    for ask in TRAILERS:
        if ask == has or not any(ask):
            continue
        asked = [n for n, on in zip(NAMES, ask) if on]
        if sum(ask) == sum(has):     # as many trailers as asked for: the container names no payload, so it reads -- and a payload's magic refuses it
            other = cu.unpack_bitstream(blob, uniform, *ask)
            assert tuple(other)[-len(asked):] == tuple(asked)
            wrong = [a for a, n in zip(asked, names) if a != n]
            with pytest.raises(ValueError, match="no b'RP[ISH]1' header"):
                getattr(cu, PARSE[wrong[0]])(bc.decompress(other[wrong[0]]), 40)
            continue
        with pytest.raises(ValueError) as e:
            cu.unpack_bitstream(blob, uniform, *ask)
        text = str(e.value)
        if sum(has) < sum(ask):                                                            # fewer trailers than asked for: the first one missing
            assert "no %s trailer" % asked[sum(has)] in text, (has, ask, text)
        elif sum(has) == 2 and asked[0] in NAMES[:2]:                                       # two trailers, one of the two older flags: the text it always had
            other = NAMES[1 - NAMES.index(asked[0])]
            assert text == ("bitstream: two trailers follow its %d payloads and only %s was asked for (compressed with --%s too? the reader needs "
                            "%s=True then)" % (len(cu.columns(uniform)), asked[0], other, other)) + "; or with --hidden_points: hidden_points=True", (has, ask, text)
        else:                                                                               # more in the blob than asked for: the flags not asked for are named
            missing = [n for n in NAMES if n not in asked]
            assert all("%s=True" % n in text and "--" + n in text for n in missing), (has, ask, text)
            assert ("one", "two", "three")[sum(has) - 1] + " trailers follow" in text
            assert (" and " if sum(has) - sum(ask) == len(missing) else " or ").join(n + "=True" for n in missing) in text
    if names:
        # every truncation of the trailers is refused by the reader that asks for them; a reader that asks for nothing still reads the geometry
        for cut in range(len(plain), len(blob)):
            with pytest.raises(ValueError):
                cu.unpack_bitstream(blob[:cut], uniform, *has)
            assert cu.unpack_bitstream(blob[:cut], uniform) == cu.unpack_bitstream(plain, uniform)
        for cut in range(len(plain)):
            with pytest.raises(ValueError):
                cu.unpack_bitstream(blob[:cut], uniform, *has)
        with pytest.raises(ValueError, match="must end the container"):
            cu.unpack_bitstream(blob + b"\0", uniform, *has)


def test_frame_slices_with_the_third_trailer():
    import torch
    import rpcc_amd  # noqa: F401
    from rpcc_amd import compress_utils as cu
    rng = np.random.default_rng(3)
    K, P, N = 5, 13, 20
    counts = np.array([[4, 0, 9, 0, 0], [13, 0, 0, 0, 0], [1, 0, 2, 0, 10]], np.int32)
    nnz, nseq = np.array([7, 0, 5], np.int32), np.array([3, 0, 4], np.int32)
    nbytes, nsub, nhid = np.array([8 + 7, 8, 8 + 5], np.int32), np.array([8 + 14, 8, 8 + 10], np.int32), np.array([16 + 7 + 4 * 11, 16, 16 + 5 + 2 * 3], np.int32)
    W = cu.HIDDEN_COLUMN.bound(P, K, N)
    assert W == 16 + P + 4 * N and cu.HIDDEN_COLUMN.name == "hidden_points" and cu.HIDDEN_COLUMN.dtype == np.uint8 and cu.HIDDEN_COLUMN.cut == "nhid"
    assert len(cu.SCHEMA) == 7 and cu.SCHEMA[-1].name == "subpixel"
    bufs = dict(salience_level=rng.integers(0, 4, (3, K)).astype(np.uint8), contour_map=rng.integers(0, 256, (3, (P + 7) // 8)).astype(np.uint8),
                idx_sequence=rng.integers(0, 9, (3 * P,)).astype(np.uint16), plane_param=rng.standard_normal((3, K, 4)).astype(np.float32),
                residual_quantized=rng.integers(-9, 9, (3 * P,)).astype(np.int16), intensity=rng.integers(0, 256, (3, 8 + P)).astype(np.uint8),
                subpixel=rng.integers(0, 4, (3, 8 + 2 * P)).astype(np.uint8), hidden_points=rng.integers(0, 256, (3, W)).astype(np.uint8))
    for has in TRAILERS:
        cols = cu.columns(False, *has)
        lens = (nbytes if has[0] else None, nsub if has[1] else None, nhid if has[2] else None)
        at = cu.frame_slices(cols, bufs, counts, nnz, nseq, *lens)
        assert list(at) == [c.name for c in cols]
        if has[2]:
            assert at["hidden_points"][0].tolist() == [0, W, 2 * W] and at["hidden_points"][1].tolist() == nhid.tolist()
            tt = cu.frame_slices(cols, {k: torch.from_numpy(v) for k, v in bufs.items()}, *(None if v is None else torch.from_numpy(v)
                                 for v in (counts, nnz, nseq) + lens))
            assert tt["hidden_points"][0].tolist() == at["hidden_points"][0].tolist() and tt["hidden_points"][1].tolist() == nhid.tolist()
            for name in at:
                assert tt[name][0].tolist() == at[name][0].tolist() and tt[name][1].tolist() == at[name][1].tolist()
        payload = cu.BatchPayload(cols, bufs, counts, nnz, nseq, lens[0], nsub=lens[1], nhid=lens[2])
        for b in range(3):
            od = payload.frame(b)
            assert cu._keys(False, od) == tuple(c.name for c in cols)
            if has[2]:
                assert od["hidden_points"].tobytes() == bufs["hidden_points"][b, : nhid[b]].tobytes() and np.shares_memory(od["hidden_points"], bufs["hidden_points"])
            if has[1]:
                assert od["subpixel"].tobytes() == bufs["subpixel"][b, : nsub[b]].tobytes()
            if has[0]:
                assert od["intensity"].tobytes() == bufs["intensity"][b, : nbytes[b]].tobytes()


# ---- C ABI -----------------------------------------------------------------------------------------------------------------------------
def test_abi_exports_and_version(built):
    hdr = open(os.path.join(ROOT, "include", "rpcc_hip.h")).read()
    lib = ctypes.CDLL(built.LIB_PATH)
    for name in ("rpcc_hidden_scratch_bytes", "rpcc_hidden_encode", "rpcc_hidden_decode"):
        assert hasattr(lib, name) and name in built.exported_symbols() and name + "(" in hdr, name
    assert "#define RPCC_STREAM_E_HIDDEN 12" in hdr and built.STREAM_E_HIDDEN == 12
    assert built.lib().rpcc_version() == built.ABI_VERSION == 105 and "#define RPCC_ABI_VERSION 105" in hdr
    need = built.lib().rpcc_hidden_scratch_bytes
    for B, P, total in ((1, 64, 0), (1, 64, 100), (3, 5000, 20000), (256, 128000, 256 * 122320)):
        n = need(B, P, total)
        assert n % 256 == 0 and n >= built.lib().rpcc_intensity_scratch_bytes(B, P) + 16 * B * P + 16 * total
        assert need(B + 1, P, total) > n and need(B, P + 64, total) > n and need(B, P, total + 64) > n
    assert need(0, 64, 10) == 0 and need(1, 0, 10) == 0 and need(65536, 64, 10) == 0 and need(1, 64, -1) == 0
    assert need(1, (1 << 30) - 4, 0) == 0 and need(1, 64, 1 << 29) == 0 and need(1, 64, (1 << 29) - 64) > 0          # 16 + P + 4 total fits an int32


def test_argument_errors_before_the_device(built):
    """Every pointer is a host dummy that must never reach a kernel: the calls return RPCC_ERR_ARG first."""
    lib = built.lib()
    dummy = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(dummy) + 255) & ~255
    geom = built.Geom(4, 16, 6.2831855, 0.03, -0.43)
    P = 64
    big = 1 << 30

    def enc(rows=p, offs=p, total=10, B=1, g=geom, ri=p, step=0.04, bits=2, payload=p, stride=16 + P + 40, nbytes=p, orphans=p, uncarried=p, scratch=p, sbytes=big):
        return lib.rpcc_hidden_encode(rows, offs, total, B, g, ri, step, bits, payload, stride, nbytes, orphans, uncarried, scratch, sbytes, None)

    need = lib.rpcc_hidden_scratch_bytes(1, P, 10)
    for kw in (dict(rows=None), dict(offs=None), dict(ri=None), dict(payload=None), dict(nbytes=None), dict(orphans=None), dict(uncarried=None), dict(scratch=None),
               dict(rows=p + 4), dict(rows=p + 8), dict(total=-1), dict(total=1 << 31), dict(total=1 << 29), dict(B=0), dict(B=65536),
               dict(g=built.Geom(1, 16, 6.28, 0.0, -0.4)), dict(g=built.Geom(0, 16, 6.28, 0.0, -0.4)), dict(g=built.Geom(4, 0, 6.28, 0.0, -0.4)),
               dict(g=built.Geom(128, 1 << 24, 6.28, 0.0, -0.4)), dict(g=built.Geom(4, 16, 0.0, 0.0, -0.4)), dict(g=built.Geom(4, 16, -6.28, 0.0, -0.4)),
               dict(g=built.Geom(4, 16, float("nan"), 0.0, -0.4)), dict(g=built.Geom(64, 1 << 24, 6.28, 0.0, -0.4), stride=1 << 40),
               dict(bits=-1), dict(bits=5), dict(bits=8), dict(step=0.0), dict(step=-0.04), dict(step=float("nan")), dict(step=float("inf")),
               dict(sbytes=need - 1), dict(sbytes=0), dict(stride=16 + P - 1), dict(stride=0), dict(stride=-5)):
        before = bytes(dummy)
        assert enc(**kw) == -1 and b"bad argument" in lib.rpcc_last_error(), kw
        assert bytes(dummy) == before

    def dec(payload=p, stride=16 + P, nbytes=p, labels=p, lb=1, tm=p, tables=p, H=4, W=16, B=1, out=p, cap=10, count=p, status=p):
        return lib.rpcc_hidden_decode(payload, stride, nbytes, labels, lb, tm, tables, H, W, B, out, cap, count, status, None)

    for kw in (dict(payload=None), dict(nbytes=None), dict(labels=None), dict(tm=None), dict(out=None), dict(count=None), dict(status=None),
               dict(lb=0), dict(lb=3), dict(lb=4), dict(B=0), dict(B=65536), dict(H=1), dict(H=0), dict(W=0), dict(H=128, W=1 << 24),
               dict(tables=p + 4), dict(cap=-1), dict(cap=1 << 31), dict(stride=15), dict(stride=0)):
        before = bytes(dummy)
        assert dec(**kw) == -1 and b"bad argument" in lib.rpcc_last_error(), kw
        assert bytes(dummy) == before


# ---- front ends --------------------------------------------------------------------------------------------------------------------------
def test_front_ends_that_refuse_hidden_points(built):
    import torch
    from rpcc_amd import compress_utils as cu
    from rpcc_amd import ops
    from rpcc_amd.loader import StreamingCompressor, StreamingDecompressor
    from rpcc_amd.pipeline import BatchCompressor, BatchDecompressor, MixedBatchCompressor
    from rpcc_amd.tools import compress as tc
    from rpcc_amd.tools import compress_datalist as tcd
    from rpcc_amd.tools import decompress_datalist as tdd
    from rpcc_amd.transformer import PCTransformer
    cfg = os.path.join(ROOT, "r-pcc_amd", "lidar_cfg")
    yaml_, csv_ = os.path.join(cfg, "Velodyne_HDL_64E.yaml"), os.path.join(cfg, "Velodyne_HDL_64E_beams.csv")
    T, E = PCTransformer(yaml_, csv_, device="cpu"), PCTransformer(yaml_, device="cpu")
    with pytest.raises(NotImplementedError, match="BatchCompressor: hidden_points with a per-beam elevation table.*last point wins"):
        BatchCompressor(T, hidden_points=True)
    with pytest.raises(NotImplementedError, match="hidden_points with a per-beam elevation table"):
        cu.encode_hidden(T, np.zeros((5, 4), np.float32), np.zeros((64, 2000), np.float32), 0.04, 0)
    with pytest.raises(NotImplementedError, match="MixedBatchCompressor: hidden_points"):
        MixedBatchCompressor({"a": E}, hidden_points=True)
    with pytest.raises(NotImplementedError, match="BatchDecompressor: hidden_points"):
        BatchDecompressor(E, 100, 0.04, hidden_points=True)
    with pytest.raises(NotImplementedError, match="StreamingDecompressor: hidden_points"):
        StreamingDecompressor(None, hidden_points=True)
    for flag in ("--batch_decode", "--stream_decode"):
        args = tc.make_parser(datalist=True).parse_args(["--datalist", "none.txt", "--output_dir", "none", "--lidar", "Velodyne64E", flag, "--hidden_points"])
        with pytest.raises(NotImplementedError, match="--%s with --hidden_points" % flag[2:]):
            tdd.decompress(args)
    # the existing refusals stay as they are
    with pytest.raises(NotImplementedError, match="MixedBatchCompressor: subpixel_bits"):
        MixedBatchCompressor({"a": E}, subpixel_bits=2, hidden_points=True)
    with pytest.raises(NotImplementedError, match="BatchDecompressor: subpixel"):
        BatchDecompressor(E, 100, 0.04, subpixel=True, hidden_points=True)
    bc = BatchCompressor(E, hidden_points=True)
    assert bc.hidden_points is True and BatchCompressor(E).hidden_points is False and [c.name for c in bc.columns][-1] == "hidden_points"
    assert [c.name for c in BatchCompressor(E).columns] == [c.name for c in cu.columns(True)]
    assert [c.name for c in BatchCompressor(E, subpixel_bits=1, intensity_scale=100, hidden_points=True).columns][-3:] == list(NAMES)
    with pytest.raises(ValueError, match='hidden_points needs ingest="rows"'):
        StreamingCompressor(bc, batch=2, ingest="xyz")
    with pytest.raises(ValueError, match="16-byte rows"):
        ops.hidden_encode(torch.zeros((5, 3)), torch.tensor([0, 5]), E.geom, torch.zeros((1, 64, 2000)), 0.04)
    for bad in (-1, 5, 2.5, "2"):
        with pytest.raises(ValueError, match="hidden_points bits"):
            ops.check_hidden_bits(bad)
    # the tools' flag
    parse = lambda *a: tc.make_parser().parse_args(["--input", "x.bin", "--output", "y.rpcc", "--lidar", "Velodyne64E"] + list(a))
    assert parse().hidden_points is False and parse("--hidden_points").hidden_points is True
    assert "The trailer carries no intensity" in " ".join(tc.make_parser().format_help().split())
    # a datalist: .bin files only, as --subpixel
    assert tcd.resolve_ingest("auto", ["a.bin", "b.bin"], hidden_points=True) == "rows"
    for want, names in (("auto", ["a.bin", "b.npy"]), ("xyz", ["a.bin"])):
        with pytest.raises(SystemExit, match="--hidden_points on a datalist needs .bin files"):
            tcd.resolve_ingest(want, names, hidden_points=True)
    assert tcd.resolve_ingest("auto", ["a.npy"]) == "xyz"
