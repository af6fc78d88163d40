"""The .rpcc container's schema (compress_utils.SCHEMA / columns), the one container walk (payload_spans) against its three callers, and
the one slicing rule (frame_slices) against BatchPayload.  No GPU."""
import struct

import numpy as np
import pytest

import rpcc_amd  # noqa: F401
from rpcc_amd import compress_utils as cu
from rpcc_amd import rans_codec
from rpcc_amd.pipeline import container_spans

GEOMETRY = ("contour_map", "idx_sequence", "plane_param", "residual_quantized")


def test_column_order():
    """The pin of the file order."""
    names = lambda uniform, intensity: tuple(c.name for c in cu.columns(uniform, intensity))
    assert names(True, False) == ("contour_map", "idx_sequence", "plane_param", "residual_quantized")
    assert names(False, False) == ("salience_level", "contour_map", "idx_sequence", "plane_param", "residual_quantized")
    assert names(True, True) == ("contour_map", "idx_sequence", "plane_param", "residual_quantized", "intensity")
    assert names(False, True) == ("salience_level", "contour_map", "idx_sequence", "plane_param", "residual_quantized", "intensity")
    assert cu._keys(True) == names(True, False) and cu._keys(False, {"intensity": b""}) == names(False, True)
    assert cu._keys(False) == names(False, False) and cu._keys(True, {"intensity": b""}) == names(True, True)


def test_widths_filter_and_bounds():
    cols = cu.columns(False, True)
    assert [c.dtype.itemsize for c in cols] == [1, 1, 2, 4, 2, 1]
    assert [c.name for c in cols if rans_codec.delta_filter(c.dtype) == rans_codec.FILTER_DELTA] == ["residual_quantized"]
    assert all(rans_codec.delta_filter(c.dtype) == rans_codec.FILTER_NONE for c in cols if c.name != "residual_quantized")
    assert [c.bound(13, 3) for c in cols] == [3, 2, 26, 48, 26, 21]          # P = 13: no multiple of 8, the packed bits round up


def _raises(blob, uniform, intensity=False):
    try:
        return cu.unpack_bitstream(blob, uniform, intensity=intensity), None
    except ValueError as e:
        return None, str(e)


@pytest.mark.parametrize("trailer", (False, True), ids=("plain", "trailer"))
@pytest.mark.parametrize("uniform", (True, False), ids=("uniform", "nonuniform"))
def test_walker_against_its_three_callers(uniform, trailer):
    keys = cu._keys(uniform, {"intensity": b""} if trailer else ())
    parts = {k: bytes([65 + i]) * (2 + 3 * i) for i, k in enumerate(keys)}
    parts["idx_sequence"] = b""                                               # an empty payload is a payload
    blob = cu.pack_bitstream(parts, uniform)
    assert blob == b"".join(struct.pack("i", len(parts[k])) + parts[k] for k in keys)
    ns = len(cu.columns(uniform))
    starts = [s - 4 for s, _ in cu.payload_spans(blob, len(keys))]
    assert len(starts) == len(keys)
    cases = [blob[:n] for n in range(len(blob) + 1)]                          # every truncation, the whole blob last
    for off in starts:                                                        # a negative prefix, and one a byte too long, at each position
        left = len(blob) - off - 4
        cases += [blob[:off] + struct.pack("i", -1) + blob[off + 4:], blob[:off] + struct.pack("i", left + 1) + blob[off + 4:]]
    seen = {"sound": 0, "refused": 0, "trailer": 0, "no trailer": 0, "ends before": 0, "claims": 0}
    for b in cases:
        spans = container_spans(b, uniform)
        got, err = _raises(b, uniform)
        assert (spans is None) == (got is None), (len(b), err)
        if spans is None:
            seen["refused"] += 1
            seen["ends before"] += "ends before the length of" in err
            seen["claims"] += " bytes, " in err and " are left" in err and "claims " in err
        else:
            seen["sound"] += 1
            assert len(spans) == ns and [b[o: o + n] for o, n in spans] == list(got.values()) and tuple(got) == keys[:ns]
        span = cu.intensity_trailer_span(b, uniform)
        got_t, err_t = _raises(b, uniform, intensity=True)
        assert (span is None) == (got_t is None), (len(b), err_t)
        if span is not None:
            seen["trailer"] += 1
            assert got_t["intensity"] == b[span[0]: span[1]] and span[1] == len(b) and tuple(got_t) == keys[:ns] + ("intensity",)
        elif got is not None:
            seen["no trailer"] += 1
            assert "no intensity trailer after its %d payloads" % ns in err_t
    assert seen["sound"] and seen["refused"] and seen["ends before"] and seen["claims"] and seen["ends before"] + seen["claims"] == seen["refused"]
    assert seen["no trailer"] and (seen["trailer"] > 0) == trailer
    if trailer:
        assert cu.unpack_bitstream(blob, uniform, intensity=True) == parts and cu.intensity_trailer_span(blob, uniform)[1] == len(blob)
    # the two texts of unpack_bitstream, word for word
    first = keys[0]
    with pytest.raises(ValueError) as e:
        cu.unpack_bitstream(blob[:3], uniform)
    assert str(e.value) == "bitstream ends before the length of '%s' (3 bytes; written with the %s framework?)" % (first, "non-uniform" if uniform else "uniform")
    with pytest.raises(ValueError) as e:
        cu.unpack_bitstream(blob[:5], uniform)
    assert str(e.value) == "bitstream: payload '%s' claims %d bytes, 1 are left" % (first, len(parts[first]))


def _batch(K=5, P=13):
    """B = 3: frame 1 has no residuals and no index sequence; frame 2's last non-zero count is at K - 1."""
    rng = np.random.default_rng(3)
    counts = np.array([[4, 0, 9, 0, 0], [13, 0, 0, 0, 0], [1, 0, 2, 0, 10]], np.int32)
    nnz, nseq, nbytes = np.array([7, 0, 5], np.int32), np.array([3, 0, 4], np.int32), np.array([8 + 7, 8, 8 + 5], np.int32)
    bufs = dict(salience_level=rng.integers(0, 4, (3, K)).astype(np.uint8), contour_map=rng.integers(0, 256, (3, (P + 7) // 8)).astype(np.uint8),
                idx_sequence=rng.integers(0, 9, (3 * P,)).astype(np.uint16), plane_param=rng.standard_normal((3, K, 4)).astype(np.float32),
                residual_quantized=rng.integers(-9, 9, (3 * P,)).astype(np.int16), intensity=rng.integers(0, 256, (3, 8 + P)).astype(np.uint8))
    return bufs, counts, nnz, nseq, nbytes


def test_slicing_rule():
    import torch
    bufs, counts, nnz, nseq, nbytes = _batch()
    cols = cu.columns(False, True)
    at = cu.frame_slices(cols, bufs, counts, nnz, nseq, nbytes)
    K, nb, row = 5, 2, 21
    want = {"salience_level": ([0, K, 2 * K], [3, 1, 5]), "contour_map": ([0, nb, 2 * nb], [nb, nb, nb]), "idx_sequence": ([0, 3, 3], [3, 0, 4]),
            "plane_param": ([0, 4 * K, 8 * K], [12, 4, 20]), "residual_quantized": ([0, 7, 7], [7, 0, 5]), "intensity": ([0, row, 2 * row], [15, 8, 13])}
    assert set(at) == set(want)
    for k, (s, n) in want.items():
        assert at[k][0].dtype == at[k][1].dtype == np.int64 and at[k][0].tolist() == s and at[k][1].tolist() == n, k
    tt = cu.frame_slices(cols, {k: torch.from_numpy(v) for k, v in bufs.items()}, *(torch.from_numpy(v) for v in (counts, nnz, nseq, nbytes)))
    for k in want:
        assert all(torch.is_tensor(t) and t.dtype == torch.int64 for t in tt[k]), k
        assert tt[k][0].tolist() == want[k][0] and tt[k][1].tolist() == want[k][1], k
    # without the salience and intensity columns nothing is asked of their buffers or counts
    plain = cu.frame_slices(cu.columns(True), dict(bufs, salience_level=None, intensity=None), counts, nnz, nseq)
    assert set(plain) == set(GEOMETRY) and all(plain[k][0].tolist() == want[k][0] and plain[k][1].tolist() == want[k][1] for k in plain)
    # the value chosen for a row of zeros, which no frame has: no rows, on the host and on the device alike
    zero = cu.frame_slices(cols, bufs, np.zeros_like(counts), nnz, nseq, nbytes)
    assert zero["plane_param"][1].tolist() == [0, 0, 0] and zero["salience_level"][1].tolist() == [0, 0, 0]


@pytest.mark.parametrize("uniform,intensity", [(True, False), (False, True)], ids=("uniform", "nonuniform+intensity"))
def test_batch_payload_returns_views_of_the_slices(uniform, intensity):
    bufs, counts, nnz, nseq, nbytes = _batch()
    cols = cu.columns(uniform, intensity)
    at = cu.frame_slices(cols, bufs, counts, nnz, nseq, nbytes)
    payload = cu.BatchPayload(cols, bufs, counts, nnz, nseq, nbytes if intensity else None)
    from rpcc_amd import loader
    assert loader.BatchPayload is cu.BatchPayload and len(payload) == 3 and len(cu.BatchPayload(cols, bufs, counts, nnz, nseq, nbytes, n=2)) == 2
    for b in range(3):
        od = payload.frame(b)
        assert set(od) == {c.name for c in cols} and cu._keys(uniform, od) == tuple(c.name for c in cols)
        for c in cols:
            s, n = int(at[c.name][0][b]), int(at[c.name][1][b])
            assert od[c.name].dtype == c.dtype and od[c.name].size == n
            assert np.array_equal(od[c.name].reshape(-1), bufs[c.name].reshape(-1)[s: s + n]), (b, c.name)
            assert np.shares_memory(od[c.name], bufs[c.name]) or n == 0, (b, c.name)
            assert od[c.name].base is not None                                # a view, not a copy
        assert od["plane_param"].shape == (at["plane_param"][1][b] // 4, 4)
