"""-m gpu: librpcc_rans.so against tests/rans_ref.py over tests/rans_cases.py: the encoder's streams byte for byte,
the decoder on the device's, the reference's and the forced-coded streams, the reference's status on every hostile stream with the output
slot left as it was, all cases as one mixed batch, exact-size buffers between guards under hostile contents, and the example sweep's
arrays at the default chunk size against their pins."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import rans_cases as C  # noqa: E402
import rans_ref as R  # noqa: E402
from buffer_arena import Arena  # noqa: E402

SIDE_PATTERNS = ("ones", "alt(0,1)", "half(0)")


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available()
    import __graft_entry__ as ge
    ge.build()
    from rpcc_amd import _rans_lib as L, rans_codec
    return dict(torch=torch, dev=torch.device("cuda:0"), L=L, codec=rans_codec)


def _encode(env, cases):
    """One rpcc_rans_encode per chunk size over [(data, width, chunk_log2)] -> the streams, in order."""
    from rpcc_amd import entropy
    torch, codec = env["torch"], env["codec"]
    out = [None] * len(cases)
    for clog in sorted({c for _, _, c in cases}):
        idx = [i for i, (_, _, c) in enumerate(cases) if c == clog]
        arrays = [np.frombuffer(cases[i][0], np.uint8) for i in idx]
        got, body, off = entropy.encode_list(arrays, env["dev"], codec.encode_descriptors, widths=[cases[i][1] for i in idx], chunk_log2=clog)
        assert (got >= 0).all()
        for i, o, g in zip(idx, off, got):
            out[i] = body[o: o + g].tobytes()
    torch.cuda.synchronize()
    return out


def test_encode_equals_reference_in_mixed_batches(env):
    """Every valid case, all cases of a chunk size in one call: widths, lengths, stored and coded forms mixed, empty streams in the middle."""
    names = list(C.everything())
    assert 0 < names.index("one_n0_w2") < len(names) - 1
    got = _encode(env, [C.everything()[k] for k in names])
    coded = 0
    for k, g in zip(names, got):
        assert g == C.reference(k), k
        coded += g[2] == 1
    assert coded >= 40


def test_golden_arrays_equal_their_pins(env):
    pins = json.load(open(os.path.join(HERE, "golden", "rans_pins.json")))
    arrays = [np.frombuffer(d, {1: np.uint8, 2: np.int16, 4: np.float32}[w]) for d, w in C.golden().values()]
    got = env["codec"].compress_many(arrays)      # widths from the arrays' itemsize, the default chunk size
    for k, g in zip(C.golden(), got):
        pin = pins["golden_" + k]
        assert (len(g), hashlib.sha256(g).hexdigest()) == (pin["length"], pin["sha256"]), k
    assert env["codec"].decompress_many(got) == [d for d, _ in C.golden().values()]


def test_decode_device_reference_and_forced_streams(env):
    codec = env["codec"]
    names = list(C.everything())
    want = [C.everything()[k][0] for k in names]
    own = _encode(env, [C.everything()[k] for k in names])
    assert codec.decompress_many(own) == want
    assert codec.decompress_many([C.reference(k) for k in names]) == want
    forced = C.forced()
    st, outs = codec.decode_many([s for s, _ in forced.values()])
    assert not st.any()
    for (k, (_, d)), o in zip(forced.items(), outs):
        assert o == d, k
    assert codec.compress(b"") == R.header(0, 1, 0, R.DEFAULT_CHUNK_LOG2) and codec.decompress(codec.compress(b"")) == b""


def test_hostile_streams_get_the_reference_status_and_write_nothing(env):
    """One call over every hostile stream with two sound ones among them; output slots pre-filled, a refused stream's left as it was."""
    torch, dev, L = env["torch"], env["dev"], env["L"]
    from rpcc_amd import entropy
    from rpcc_amd._lib import ptr, stream
    base, data, _ = C.base()
    rows = [("sound_first", base, len(data))] + [(k, s, cap) for k, (s, cap) in C.hostile().items()] + [("sound_last", base, len(data))]
    arrays = [np.frombuffer(s, np.uint8) for _, s, _ in rows]
    cap = np.array([c for _, _, c in rows], np.int64)
    up, offs = entropy.upload(arrays, dev)
    doff, dend = entropy.aligned_slots(cap)
    meta = torch.from_numpy(np.stack([up.data_ptr() + offs, [a.size for a in arrays], doff, cap]).astype(np.int64)).to(dev)
    n = len(rows)
    for fill in (0x00, 0xFF):
        dst = torch.full((dend,), fill, dtype=torch.uint8, device=dev)
        dst_len = torch.full((n,), -99, dtype=torch.int64, device=dev)
        status = torch.full((n,), -99, dtype=torch.int32, device=dev)
        L.check(L.lib().rpcc_rans_decode(ptr(meta[0]), ptr(meta[1]), n, ptr(dst), ptr(meta[2]), ptr(meta[3]), ptr(dst_len), ptr(status), stream()))
        st, ln, h = status.cpu().numpy(), dst_len.cpu().numpy(), dst.cpu().numpy()
        written = np.zeros(dend, bool)
        for i, (k, s, c) in enumerate(rows):
            want_st, want = R.decode(s, cap=c)
            assert (st[i], ln[i]) == (want_st, len(want)), (k, R.NAMES.get(int(st[i]), st[i]), R.NAMES[want_st])
            assert (want_st != R.OK) == (not k.startswith("sound")), k
            assert h[doff[i]: doff[i] + len(want)].tobytes() == want, k
            written[doff[i]: doff[i] + len(want)] = True
        assert (h[~written] == fill).all()           # refused streams' slots and the gaps between slots
    with pytest.raises(ValueError, match="rans stream 1"):
        env["codec"].decompress_many([base, C.hostile()["payload_word_flipped"][0]])


def test_exact_size_buffers_between_guards(env):
    """dst, ws and the decoder's output as arenas of exactly the stated sizes under hostile contents: the streams equal the reference's, the
    gaps between slots and the guards are left alone."""
    torch, dev, L, codec = env["torch"], env["dev"], env["L"], env["codec"]
    from rpcc_amd import entropy
    from rpcc_amd._lib import ptr, stream
    names = ["c10_int16_n2113_w2", "one_n0_w1", "c10_float32_n1000_w4", "random_n257_w2", "c9_dominant_n1027_w1", "c10_two_n2113_w4"]
    clog = 10
    cases = [(C.valid()[k][0], C.valid()[k][1]) for k in names]
    want = [R.encode(d, w, clog) for d, w in cases]
    assert {s[2] for s in want} == {0, 1}
    arrays = [np.frombuffer(d, np.uint8) for d, _ in cases]
    up, offs = entropy.upload(arrays, dev)
    n = len(cases)
    lens = np.array([a.size for a in arrays], np.int64)
    desc = torch.from_numpy(np.stack([up.data_ptr() + offs, lens]).astype(np.int64)).to(dev)
    widths = torch.tensor([w for _, w in cases], dtype=torch.int32, device=dev)
    cap = lens + R.HEADER
    off, end = entropy.aligned_slots(cap)
    meta = torch.from_numpy(np.stack([off, cap])).to(dev)
    total = int(lens.sum())
    enc, dec = Arena(end, dev), Arena(entropy.aligned_slots(lens)[1], dev)
    ws = Arena(int(L.lib().rpcc_rans_workspace_bytes(n, total, clog)), dev)
    doff = entropy.aligned_slots(lens)[0]
    dmeta = torch.from_numpy(np.stack([doff, lens])).to(dev)
    for pattern in SIDE_PATTERNS:
        enc.fill(pattern), dec.fill(pattern), ws.fill(pattern)
        before, dbefore = enc.view.cpu().numpy().copy(), dec.view.cpu().numpy().copy()
        dst_len = torch.full((n,), -99, dtype=torch.int64, device=dev)
        L.check(L.lib().rpcc_rans_encode(ptr(desc[0]), ptr(desc[1]), ptr(widths), n, total, clog, ptr(enc.view), ptr(meta[0]), ptr(meta[1]),
                                         ptr(dst_len), ptr(ws.view), stream()))
        got, h = dst_len.cpu().numpy(), enc.view.cpu().numpy()
        keep = np.ones(h.size, bool)
        for k in range(n):
            assert h[off[k]: off[k] + got[k]].tobytes() == want[k], (pattern, names[k])
            keep[off[k]: off[k] + got[k]] = False
        assert np.array_equal(h[keep], before[keep]), pattern
        sdesc = torch.tensor([[enc.view.data_ptr() + int(o) for o in off], got.tolist()], dtype=torch.int64, device=dev)
        out_len = torch.full((n,), -99, dtype=torch.int64, device=dev)
        status = torch.full((n,), -99, dtype=torch.int32, device=dev)
        L.check(L.lib().rpcc_rans_decode(ptr(sdesc[0]), ptr(sdesc[1]), n, ptr(dec.view), ptr(dmeta[0]), ptr(dmeta[1]), ptr(out_len), ptr(status), stream()))
        assert not status.cpu().numpy().any() and np.array_equal(out_len.cpu().numpy(), lens), pattern
        hd, dkeep = dec.view.cpu().numpy(), np.ones(dec.nbytes, bool)
        for k in range(n):
            assert hd[doff[k]: doff[k] + lens[k]].tobytes() == cases[k][0], (pattern, names[k])
            dkeep[doff[k]: doff[k] + lens[k]] = False
        assert np.array_equal(hd[dkeep], dbefore[dkeep]), pattern
        for a, what in ((enc, "dst"), (dec, "decoded"), (ws, "ws")):
            assert a.check_guards() is None, (what, pattern, a.check_guards())


def test_encoder_refuses_what_does_not_fit(env):
    """A slot below 12 + n, a width of 3 and a length beyond total_bytes are refused per stream (E_CAPACITY, nothing written); the others code."""
    torch, dev, L = env["torch"], env["dev"], env["L"]
    from rpcc_amd import entropy
    from rpcc_amd._lib import ptr, stream
    data, long = C.valid()["c10_int16_n2113_w2"][0], C.valid()["c12_int16_n12293_w2"][0]
    arrays = [np.frombuffer(data, np.uint8)] * 3 + [np.frombuffer(long, np.uint8)]
    up, offs = entropy.upload(arrays, dev)
    lens = np.array([a.size for a in arrays], np.int64)
    desc = torch.from_numpy(np.stack([up.data_ptr() + offs, lens]).astype(np.int64)).to(dev)
    widths = torch.tensor([2, 3, 2, 2], dtype=torch.int32, device=dev)
    cap = lens + R.HEADER
    cap[2] -= 1
    off, end = entropy.aligned_slots(cap)
    meta = torch.from_numpy(np.stack([off, cap])).to(dev)
    total = 0                         # 4 groups of four 1 KiB chunks are bounded: one for the first stream, the last one needs four
    ws = torch.empty(int(L.lib().rpcc_rans_workspace_bytes(4, total, 10)) + 16, dtype=torch.uint8, device=dev)
    ws = ws[(-ws.data_ptr()) % 16:]
    dst = torch.full((end,), 0x5A, dtype=torch.uint8, device=dev)
    dst_len = torch.full((4,), -99, dtype=torch.int64, device=dev)
    L.check(L.lib().rpcc_rans_encode(ptr(desc[0]), ptr(desc[1]), ptr(widths), 4, total, 10, ptr(dst), ptr(meta[0]), ptr(meta[1]), ptr(dst_len),
                                     ptr(ws), stream()))
    got, h = dst_len.cpu().numpy(), dst.cpu().numpy()
    want = R.encode(data, 2, 10)
    assert got[0] == len(want) and h[: got[0]].tobytes() == want
    assert got[1] == got[2] == got[3] == L.E_CAPACITY
    assert (h[got[0]:] == 0x5A).all()
