"""-m gpu: librpcc_bunzip2.so against bz2.decompress and tests/bunzip2_ref.py: the same bytes on every valid
stream, the reference's status, size and input count on every malformed one, the E_OVERRUN retry, the caller-buffer contract, and
basic_compressor 'bzip2' with device_bunzip2 through BasicCompressor and the tools."""
import bz2
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import buffer_arena as BA  # noqa: E402
import bunzip2_cases as C  # noqa: E402
import bunzip2_ref as R  # noqa: E402

GAP = 0xA5


@pytest.fixture(scope="module")
def codec():
    import torch
    assert torch.cuda.is_available()
    import __graft_entry__ as ge
    ge.build()
    from rpcc_amd import bunzip2_codec
    return bunzip2_codec


def _sources(streams, dev):
    """The streams in one device buffer, every one at an odd address.  -> (buffer, addr i64 [n], len i64 [n]) (numpy for the last two)."""
    import torch
    off, at = [], 1
    for s in streams:
        off.append(at)
        at += len(s) + 1 + (len(s) & 1)        # odd + even stays odd
    host = np.zeros(at + 1, np.uint8)
    for s, o in zip(streams, off):
        host[o: o + len(s)] = np.frombuffer(s, np.uint8)
    buf = torch.from_numpy(host).to(dev)
    assert buf.data_ptr() % 2 == 0                  # an allocation's address is even: the odd offsets make odd addresses
    return buf, np.array([buf.data_ptr() + o for o in off], np.int64), np.array([len(s) for s in streams], np.int64)


def _decode(codec, streams, caps, slots, gap=3):
    """One launch over the streams: slot s of exactly caps[s] bytes at an odd dst_off with `gap` bytes of GAP or more between the slots;
    work slot s of exactly work_bytes(slots[s]) bytes at a multiple of 4, 4 bytes of GAP or more between them.
    -> (status, dst_len, src_used, dst bytes, dst_off, work bytes, work_off, work_cap) as numpy."""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    buf, addr, lens = _sources(streams, dev)
    caps = np.asarray(caps, np.int64)
    off, at = [], 1
    for c in caps:
        off.append(at)
        at += int(c) + gap
        at += 1 - (at & 1)
    off = np.array(off, np.int64)
    dst = torch.full((at + 1,), GAP, dtype=torch.uint8, device=dev)
    wcap = np.array([codec.work_bytes(m) for m in slots], np.int64)
    woff, wat = [], 4
    for c in wcap:
        woff.append(wat)
        wat += (int(c) + 3) // 4 * 4 + 4
    woff = np.array(woff, np.int64)
    work = torch.full((wat + 4,), GAP, dtype=torch.uint8, device=dev)
    meta = torch.from_numpy(np.stack([addr, lens, off, caps, woff, wcap])).to(dev)
    dst_len, src_used, status = codec.decode_descriptors(meta[0], meta[1], dst, meta[2], meta[3], work, meta[4], meta[5])
    torch.cuda.synchronize()
    assert buf.numel()
    return status.cpu().numpy(), dst_len.cpu().numpy(), src_used.cpu().numpy(), dst.cpu().numpy(), off, work.cpu().numpy(), woff, wcap


def _untouched_outside(h, off, lens):
    keep = np.ones(h.size, bool)
    for o, l in zip(off, lens):
        keep[o: o + l] = False
    return bool((h[keep] == GAP).all())


def test_valid_streams_in_one_launch(codec):
    cases = C.valid()
    streams = [v[0] for v in cases.values()]
    plains = [v[1] for v in cases.values()]
    slots = [R.block_bound(int(s[3:4]), len(p)) for s, p in zip(streams, plains)]
    st, lens, used, h, off, w, woff, wcap = _decode(codec, streams, [len(p) for p in plains], slots)
    for k, name in enumerate(cases):
        assert st[k] == R.OK, (name, R.NAMES.get(int(st[k]), st[k]))
        assert lens[k] == len(plains[k]) and used[k] == len(streams[k]), name
        got = h[off[k]: off[k] + lens[k]].tobytes()
        if got != plains[k]:
            bad = next(i for i, (a, b) in enumerate(zip(got, plains[k])) if a != b)
            raise AssertionError("%s: first difference at byte %d of %d" % (name, bad, len(got)))
        assert got == bz2.decompress(streams[k]), name
    assert _untouched_outside(h, off, lens) and _untouched_outside(w, woff, wcap)


@functools.lru_cache(maxsize=None)
def _malformed():
    """-> [(name, stream, dst_cap, work block, the reference's (status, bytes, size, src_used))]"""
    rows = [("flip%d" % k, s, C.FLIP_CAP, C.FLIP_BLOCK) for k, s in enumerate(C.flips())]
    rows += [("cut%d" % k, s, C.FLIP_CAP, C.FLIP_BLOCK) for k, s in enumerate(C.truncations())]
    rows += [(name, s, cap, slot) for name, (s, cap, slot, _) in C.hand_built().items()] + [("empty", b"", 0, 0)]
    return [(name, s, cap, slot, R.bunzip2(s, cap=cap, nblock_max=slot)) for name, s, cap, slot in rows]


def test_malformed_streams_in_one_launch(codec):
    rows = _malformed()
    assert len(rows) > 1200
    st, lens, used, h, off, w, woff, wcap = _decode(codec, [r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows])
    wrong = [(name, R.NAMES.get(int(st[k]), int(st[k])), R.NAMES[want[0]]) for k, (name, _, _, _, want) in enumerate(rows) if st[k] != want[0]]
    assert not wrong, (len(wrong), wrong[:10])
    hand = C.hand_built()
    for k, (name, s, cap, slot, want) in enumerate(rows):
        assert (lens[k], used[k]) == (want[2], want[3]), name
        if want[0] in (R.OK, R.E_OVERRUN):
            assert h[off[k]: off[k] + len(want[1])].tobytes() == want[1], name
        if want[0] == R.OK:
            assert want[1] == bz2.decompress(s), name
        if name in hand and hand[name][3] is not None:
            assert st[k] == hand[name][3], name
    assert _untouched_outside(h, off, [r[2] for r in rows])       # nothing outside the slots, whatever the stream
    assert _untouched_outside(w, woff, wcap)


def test_overrun_reports_the_size_and_the_retry_decodes(codec):
    v = C.valid()
    names = ["golden_idx_sequence", "run259", "random_level1", "all_bytes"]
    streams = [v[n][0] for n in names]
    plains = [v[n][1] for n in names]
    short = [len(p) - 1 for p in plains]
    slots = [100000 * int(s[3:4]) for s in streams]
    st, lens, used, h, off, _, _, _ = _decode(codec, streams, short, slots)
    assert st.tolist() == [R.E_OVERRUN] * 4 and lens.tolist() == [len(p) for p in plains] and used.tolist() == [len(s) for s in streams]
    for k, p in enumerate(plains):
        assert h[off[k]: off[k] + short[k]].tobytes() == p[:-1]
    assert _untouched_outside(h, off, short)
    st, lens2, _, h, off, _, _, _ = _decode(codec, streams, lens, [R.block_bound(int(s[3:4]), n) for s, n in zip(streams, lens)])
    assert st.tolist() == [R.OK] * 4 and lens2.tolist() == lens.tolist()
    for k, p in enumerate(plains):
        assert h[off[k]: off[k] + lens2[k]].tobytes() == p


def test_caller_buffer_contract(codec):
    """dst and work are Arenas of exactly the summed slots between guards; the work slots hold poison, another one in the second run."""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    v, hb = C.valid(), C.hand_built()
    items = [(v["golden_contour_map"][0], 16000, R.OK), (hb["one_byte_over"][0], hb["one_byte_over"][1], R.E_OVERRUN),
             (v["golden_idx_sequence"][0], 12134, R.OK), (hb["block_crc"][0], 400, R.E_CRC), (v["abc_period"][0], 6000, R.OK),
             (v["abc_period"][0], 5999, R.E_OVERRUN), (v["zeros70000"][0], 70000, R.OK), (hb["three_blocks"][0], 451, R.OK),
             (hb["no_blocks"][0], 1, R.OK), (v["all_bytes"][0], 768, R.OK), (hb["slot_one_short"][0], 400, R.OK)]
    caps = np.array([c for _, c, _ in items], np.int64)
    off = np.zeros(len(items), np.int64)
    off[1:] = np.cumsum(caps)[:-1]
    assert (off & 1).any()
    blocks = [R.block_bound(int(s[3:4]), c) for s, c, _ in items]
    wcap = np.array([codec.work_bytes(b) for b in blocks], np.int64)
    woff = np.zeros(len(items), np.int64)
    woff[1:] = np.cumsum((wcap + 3) // 4 * 4)[:-1]
    arena, warena = BA.Arena(int(caps.sum()), device=dev), BA.Arena(int(woff[-1] + wcap[-1]), device=dev)
    buf, addr, lens = _sources([s for s, _, _ in items], dev)
    meta = torch.from_numpy(np.stack([addr, lens, off, caps, woff, wcap])).to(dev)

    def run(fill):
        arena.raw.fill_(BA.GUARD_BYTE)
        arena.view.fill_(fill)
        warena.fill("ones" if fill else "alt(0,1)")
        from rpcc_amd import _bunzip2_lib as L
        from rpcc_amd._lib import ptr, stream
        outs = {k: BA.filled((len(items),), t, dev, fill) for k, t in (("dst_len", torch.int64), ("src_used", torch.int64), ("status", torch.int32))}
        L.check(L.lib().rpcc_bunzip2_decode(ptr(meta[0]), ptr(meta[1]), len(items), ptr(arena.view), ptr(meta[2]), ptr(meta[3]), ptr(warena.view),
                                            ptr(meta[4]), ptr(meta[5]), ptr(outs["dst_len"]), ptr(outs["src_used"]), ptr(outs["status"]), stream()))
        torch.cuda.synchronize()
        assert arena.check_guards() is None, arena.check_guards()
        assert warena.check_guards() is None, warena.check_guards()
        return dict(outs, dst=arena.view.clone())

    outs = {}
    holes = BA.unwritten(run, outs)
    assert not holes["dst_len"].any() and not holes["status"].any() and not holes["src_used"].any()      # written for every stream
    st, got = outs["status"].cpu().numpy(), outs["dst_len"].cpu().numpy()
    assert st.tolist() == [w for _, _, w in items]
    assert buf.numel()
    hole = holes["dst"].cpu().numpy()
    data = outs["dst"].cpu().numpy()
    for k, (s, cap, want) in enumerate(items):
        slot = hole[off[k]: off[k] + cap]
        plain = bz2.decompress(s) if want != R.E_CRC else None
        if want == R.OK:
            assert got[k] == len(plain) and data[off[k]: off[k] + got[k]].tobytes() == plain, k
            assert not slot[: got[k]].any() and slot[got[k]:].all(), k     # exactly dst_len bytes written, the same in both runs
        elif want == R.E_OVERRUN:
            assert got[k] == len(plain) > cap and not slot.any() and data[off[k]: off[k] + cap].tobytes() == plain[:cap], k


def _example_arrays():
    return {k: C.valid()["golden_" + k][1] for k in C.golden_members()}


def _count_launches(codec, monkeypatch):
    calls = []
    monkeypatch.setattr(codec, "_launch", lambda arrays, cap, blocks, dev, f=codec._launch: calls.append(len(arrays)) or f(arrays, cap, blocks, dev))
    return calls


def test_basic_compressor_device_bunzip2(codec, monkeypatch):
    from rpcc_amd import compress_utils as cu
    bc, host = cu.BasicCompressor(method_name="bzip2", device_bunzip2=True), cu.BasicCompressor(method_name="bzip2")
    assert bc.batch_decoder() is codec.decompress_many and host.batch_decoder() is None
    blobs = dict(C.golden_members())
    want = _example_arrays()
    calls = _count_launches(codec, monkeypatch)
    assert bc.decompress_dict(blobs) == want == host.decompress_dict(blobs)
    assert calls == [4]                                     # the guess holds for this project's payloads: one launch
    assert list(bc.decompress_dict(blobs)) == list(blobs)
    del calls[:]
    assert bc.decompress(blobs["residual_quantized"]) == want["residual_quantized"] == host.decompress(blobs["residual_quantized"])
    frames = [blobs, {"x": bz2.compress(b"abc" * 500, 1), "y": bz2.compress(b"")}, {k: blobs[k] for k in list(blobs)[:2]}]
    assert bc.decompress_dicts(frames) == [host.decompress_dict(f) for f in frames] == host.decompress_dicts(frames)
    assert calls == [1, 8]
    assert bc.decompress_dicts([]) == []
    a = np.arange(5000, dtype=np.int16) % 37
    assert bc.compress(a) == bz2.compress(a)                # compression is bz2.compress under every flag
    del calls[:]
    # what the guess does not cover: 70000 zero bytes from 47 (one more launch at the size the first reports); what the kernel leaves to
    # libbz2: a second stream, trailing bytes, the empty blob
    two = bz2.compress(b"one ") + bz2.compress(b"two")
    odd = [C.valid()["zeros70000"][0], two, blobs["plane_param"] + bytes(3), b"", C.hand_built()["randomised"][0]]
    assert codec.decompress_many(odd) == [bz2.decompress(s) for s in odd]
    assert calls == [5, 1]
    bad = bytearray(blobs["idx_sequence"])
    bad[len(bad) // 2] ^= 0x10
    with pytest.raises(ValueError, match=r"bzip2 stream 1: .*\(status -\d+\)"):
        bc.decompress_dict({"contour_map": blobs["contour_map"], "idx_sequence": bytes(bad)})
    st, outs = codec.decode_many([blobs["plane_param"], blobs["plane_param"]], caps=[1632, 1631])
    assert st.tolist() == [R.OK, R.E_OVERRUN] and outs == [want["plane_param"], None]


def test_work_slot_retry_is_the_third_launch(codec, monkeypatch):
    """A stream whose guessed capacity is far too small: the work slot sized from it cannot hold the block (E_WORK), the launch with the
    level's block reports the size (E_OVERRUN), the third decodes."""
    rng = np.random.default_rng(3)
    plain = bytes(rng.integers(0, 2, 8, dtype=np.uint8)) * 40000          # 320000 bytes that shrink about a thousand times
    s = bz2.compress(plain)
    assert len(s) * codec.GUESS_RATIO + codec.GUESS_SLACK < len(plain) // 40
    calls = _count_launches(codec, monkeypatch)
    assert codec.decompress_many([s, C.golden_members()["plane_param"]]) == [plain, _example_arrays()["plane_param"]]
    assert calls == [2, 1, 1]


def _example_rpcc(tmp_path):
    z = np.load(os.path.join(HERE, "golden", "example_64E.npz"))
    out = tmp_path / "frame.rpcc"
    out.write_bytes(z["rpcc"].tobytes())
    return out


def test_decompress_tool(codec, tmp_path, monkeypatch):
    """tools/decompress.py on the golden example_64E container (bzip2, the default), with and without --device_bunzip2: the same
    reconstruction; with the flag the frame's four arrays go through bunzip2_codec in one launch."""
    from rpcc_amd.tools import decompress as td
    src = _example_rpcc(tmp_path)
    calls = _count_launches(codec, monkeypatch)
    recs = {}
    for flag in ([], ["--device_bunzip2"]):
        rec = tmp_path / ("rec%d.npy" % len(flag))
        td.decompress(td.make_parser().parse_args(["--input", str(src), "--output", str(rec), "--lidar", "Velodyne64E"] + flag))
        recs[len(flag)] = np.load(rec)
        assert calls == ([] if not flag else [4])
    assert recs[0].shape[0] > 10000 and np.array_equal(recs[0], recs[1])


def test_decompress_datalist_tool(codec, tmp_path, monkeypatch):
    """tools/decompress_datalist.py over three .rpcc files, in chunks of two: the same .bin bytes with and without --device_bunzip2."""
    from oracle import oracle as orc
    from rpcc_amd import synth
    from rpcc_amd.tools import compress as tc
    from rpcc_amd.tools import decompress_datalist as tdl
    gd = orc.GEOMS["VelodyneVLP16"]
    base = ["--lidar", "VelodyneVLP16", "--basic_compressor", "bzip2"]
    names = []
    for k in range(3):
        f = synth.make_frame(60 + k, gd["H"], gd["W"], vmax_deg=gd["vmax_deg"], vmin_deg=gd["vmin_deg"]).numpy()
        src, out = tmp_path / ("sweep%d.bin" % k), tmp_path / ("packed%d.rpcc" % k)
        np.concatenate((f, np.zeros((f.shape[0], 1), np.float32)), 1).astype(np.float32).tofile(src)
        tc.compress(tc.make_parser().parse_args(["--input", str(src), "--output", str(out)] + base))
        names.append(str(out))
    lst = tmp_path / "list.txt"
    lst.write_text("\n".join(names) + "\n")
    calls = _count_launches(codec, monkeypatch)
    monkeypatch.setattr(tdl, "CHUNK", 2)
    files = {}
    for flag in ([], ["--device_bunzip2"]):
        od = tmp_path / ("out%d" % len(flag))
        tdl.decompress(tc.make_parser(datalist=True).parse_args(["--datalist", str(lst), "--output_dir", str(od)] + base + flag))
        files[len(flag)] = {os.path.basename(f): open(os.path.join(d, f), "rb").read() for d, _, fs in os.walk(od) for f in fs}
    assert calls == [8, 4]                               # chunks of two frames and of one, four arrays each, one launch per chunk
    assert sorted(files[0]) == ["packed%d.bin" % k for k in range(3)] and files[0] == files[1]
    assert len(set(files[0].values())) == 3 and all(len(v) > 10000 for v in files[0].values())
