"""-m gpu: version 2 of the 'rans' format (the delta filter) in librpcc_rans.so against tests/rans_filter_ref.py over
tests/rans_filter_cases.py: the encoder's streams byte for byte with filtered, unfiltered, stored and empty
streams in one call, the decoder on the device's, the reference's and the forced-coded streams, bad width words refused beside streams
that code, the reference's status on every hostile 'RB' stream with the output slot left as it was, and exact-size buffers between guards
under hostile contents."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import rans_filter_cases as C  # noqa: E402
import rans_filter_ref as F  # noqa: E402
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
    """One rpcc_rans_encode per chunk size over [(data, width, chunk_log2, filter)] -> the streams, in order."""
    from rpcc_amd import entropy
    torch, codec = env["torch"], env["codec"]
    out = [None] * len(cases)
    for clog in sorted({c[2] for c in cases}):
        idx = [i for i, c in enumerate(cases) if c[2] == clog]
        arrays = [np.frombuffer(cases[i][0], np.uint8) for i in idx]
        got, body, off = entropy.encode_list(arrays, env["dev"], codec.encode_descriptors, widths=[cases[i][1] for i in idx],
                                             filters=[cases[i][3] for i in idx], chunk_log2=clog)
        assert (got >= 0).all()
        for i, o, g in zip(idx, off, got):
            out[i] = body[o: o + g].tobytes()
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def own(env):
    """The device's streams of every case, all cases of a chunk size in one call."""
    return dict(zip(C.valid(), _encode(env, list(C.valid().values()))))


def test_encode_equals_reference_in_mixed_batches(own):
    """Filtered and unfiltered, coded and stored, empty streams in the middle: every stream is the reference's."""
    names = list(C.valid())
    assert 0 < names.index("c9_walk_n0_w2") < len(names) - 1
    forms = {}
    for k in names:
        assert own[k] == C.reference(k), k
        key = (own[k][:2], own[k][2], C.valid()[k][3])
        forms[key] = forms.get(key, 0) + 1
    assert forms[(b"RB", 1, 1)] >= 60                 # the filtered coded path
    assert forms[(b"RA", 0, 1)] >= 30                 # a filtered stream that would not shrink: the version-1 stored stream
    assert forms[(b"RA", 1, 0)] >= 3                  # unfiltered beside them


def test_a_filtered_stream_that_would_not_shrink_is_stored_as_version_1(own):
    for k in ("c10_random_n2049_w2", "c9_walk_n63_w4", "c9_walk_n1_w1"):
        d, w, c, f = C.valid()[k]
        assert f == F.FILTER_DELTA and own[k] == R.header(0, w, len(d), c) + d, k


def test_decode_device_reference_and_forced_streams(env, own):
    codec = env["codec"]
    names = list(C.valid())
    want = [C.valid()[k][0] for k in names]
    assert codec.decompress_many([own[k] for k in names]) == want
    assert codec.decompress_many([C.reference(k) for k in names]) == want
    forced = C.forced()
    st, outs = codec.decode_many([s for s, _ in forced.values()])
    assert not st.any()
    for (k, (s, d)), o in zip(forced.items(), outs):
        assert s[:2] == b"RB" and o == d, k


def test_bad_width_words_are_refused_beside_streams_that_code(env):
    """0x0202 (filter 2), 0x0103 (width 3), 0x10002 (a higher bit) and -1: E_CAPACITY for that stream, nothing written; its neighbours code."""
    torch, dev, L = env["torch"], env["dev"], env["L"]
    from rpcc_amd import entropy
    from rpcc_amd._lib import ptr, stream
    data, w, clog, _ = C.valid()["c10_walk_n2049_w2"]
    words = [L.width_word(2, L.FILTER_DELTA), 0x0202, 2, 0x0103, L.width_word(2, L.FILTER_DELTA), 0x10002, -1, 0x0102]
    assert words[0] == words[-1] == 0x0102
    n = len(words)
    arrays = [np.frombuffer(data, np.uint8)] * n
    up, offs = entropy.upload(arrays, dev)
    lens = np.array([a.size for a in arrays], np.int64)
    desc = torch.from_numpy(np.stack([up.data_ptr() + offs, lens]).astype(np.int64)).to(dev)
    widths = torch.tensor(words, dtype=torch.int32, device=dev)
    cap = lens + R.HEADER
    off, end = entropy.aligned_slots(cap)
    meta = torch.from_numpy(np.stack([off, cap])).to(dev)
    total = int(lens.sum())
    ws = entropy.work_buffer(int(L.lib().rpcc_rans_workspace_bytes(n, total, clog)), 16, dev)
    dst = torch.full((end,), 0x5A, dtype=torch.uint8, device=dev)
    dst_len = torch.full((n,), -99, dtype=torch.int64, device=dev)
    L.check(L.lib().rpcc_rans_encode(ptr(desc[0]), ptr(desc[1]), ptr(widths), n, total, clog, ptr(dst), ptr(meta[0]), ptr(meta[1]), ptr(dst_len),
                                     ptr(ws), stream()))
    got, h = dst_len.cpu().numpy(), dst.cpu().numpy()
    want = {0x0102: F.encode(data, 2, clog, F.FILTER_DELTA), 2: R.encode(data, 2, clog)}
    assert want[0x0102][:2] == b"RB" and want[2][:3] == b"RA\x01"
    keep = np.ones(end, bool)
    for k, word in enumerate(words):
        if word in want:
            assert h[off[k]: off[k] + got[k]].tobytes() == want[word], k
            keep[off[k]: off[k] + got[k]] = False
        else:
            assert got[k] == L.E_CAPACITY, (k, hex(word & 0xFFFFFFFF))
    assert (h[keep] == 0x5A).all()


def test_hostile_streams_get_the_reference_status_and_write_nothing(env):
    """One call over every hostile 'RB' stream with two sound ones among them; output slots pre-filled, a refused stream's left as it was."""
    torch, dev, L = env["torch"], env["dev"], env["L"]
    from rpcc_amd import entropy
    from rpcc_amd._lib import ptr, stream
    base, data = C.base()
    rows = [("sound_first", base, len(data))] + [(k, s, cap) for k, (s, cap) in C.hostile().items()] + [("sound_last", base, len(data))]
    arrays = [np.frombuffer(s, np.uint8) for _, s, _ in rows]
    cap = np.array([c for _, _, c in rows], np.int64)
    up, offs = entropy.upload(arrays, dev)
    doff, dend = entropy.aligned_slots(cap)
    meta = torch.from_numpy(np.stack([up.data_ptr() + offs, [a.size for a in arrays], doff, cap]).astype(np.int64)).to(dev)
    n = len(rows)
    want_all = [F.decode(s, cap=c) for _, s, c in rows]
    for fill in (0x00, 0xFF):
        dst = torch.full((dend,), fill, dtype=torch.uint8, device=dev)
        dst_len = torch.full((n,), -99, dtype=torch.int64, device=dev)
        status = torch.full((n,), -99, dtype=torch.int32, device=dev)
        L.check(L.lib().rpcc_rans_decode(ptr(meta[0]), ptr(meta[1]), n, ptr(dst), ptr(meta[2]), ptr(meta[3]), ptr(dst_len), ptr(status), stream()))
        st, ln, h = status.cpu().numpy(), dst_len.cpu().numpy(), dst.cpu().numpy()
        written = np.zeros(dend, bool)
        for i, ((k, s, c), (want_st, want)) in enumerate(zip(rows, want_all)):
            assert (st[i], ln[i]) == (want_st, len(want)), (k, R.NAMES.get(int(st[i]), st[i]), R.NAMES[want_st])
            assert (want_st != R.OK) == (not k.startswith("sound")), k
            assert h[doff[i]: doff[i] + len(want)].tobytes() == want, k
            written[doff[i]: doff[i] + len(want)] = True
        assert (h[~written] == fill).all()           # refused streams' slots and the gaps between slots
    with pytest.raises(ValueError, match="rans stream 1"):
        env["codec"].decompress_many([base, C.hostile()["filter_2"][0]])


def test_exact_size_buffers_between_guards(env):
    """dst, ws and the decoder's output as arenas of exactly the stated sizes under hostile contents, filtered and unfiltered streams of
    every width and an empty one in one call: the streams equal the reference's, the gaps between slots and the guards are left alone."""
    torch, dev, L = env["torch"], env["dev"], env["L"]
    from rpcc_amd import entropy
    from rpcc_amd._lib import ptr, stream
    names = ["c10_walk_n2049_w2", "c9_walk_n0_w1", "c10_alt_n1028_w4", "c10_random_n2049_w2", "c10_plain_n2049_w2", "c10_half_n1023_w1",
             "c10_ramp_n1020_w4", "c10_equal_n65_w2"]
    clog = 10
    cases = [C.valid()[k] for k in names]
    want = [F.encode(d, w, clog, f) for d, w, _, f in cases]
    assert {(s[:2], s[2]) for s in want} == {(b"RA", 0), (b"RA", 1), (b"RB", 1)}
    arrays = [np.frombuffer(c[0], np.uint8) for c in cases]
    up, offs = entropy.upload(arrays, dev)
    n = len(cases)
    lens = np.array([a.size for a in arrays], np.int64)
    desc = torch.from_numpy(np.stack([up.data_ptr() + offs, lens]).astype(np.int64)).to(dev)
    widths = torch.tensor([L.width_word(c[1], c[3]) for c in cases], dtype=torch.int32, device=dev)
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
