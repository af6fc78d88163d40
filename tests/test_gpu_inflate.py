"""-m gpu: librpcc_inflate.so against gzip.decompress and tests/inflate_ref.py: the same bytes on every valid
stream, the reference's status on every malformed one -- OK exactly where gzip.decompress returns -- the caller-buffer contract, and
basic_compressor 'deflate' with device_entropy on the way back through BasicCompressor and the tools."""
import functools
import gzip
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import buffer_arena as BA  # noqa: E402
import inflate_cases as C  # noqa: E402
import inflate_ref as R  # noqa: E402

GAP = 0xA5


@pytest.fixture(scope="module")
def codec():
    import torch
    assert torch.cuda.is_available()
    import __graft_entry__ as ge
    ge.build()
    from rpcc_amd import inflate_codec
    return inflate_codec


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


def _decode(codec, streams, caps, gap=3):
    """One launch over the streams: slot s of exactly caps[s] bytes at an odd dst_off, `gap` bytes of GAP or more between the slots.
    -> (status, dst_len, dst bytes, dst_off) as numpy."""
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
    meta = torch.from_numpy(np.stack([addr, lens, off, caps])).to(dev)
    dst_len, status = codec.decode_descriptors(meta[0], meta[1], dst, meta[2], meta[3])
    torch.cuda.synchronize()
    assert buf.numel()
    return status.cpu().numpy(), dst_len.cpu().numpy(), dst.cpu().numpy(), off


def _untouched_outside(h, off, lens):
    keep = np.ones(h.size, bool)
    for o, l in zip(off, lens):
        keep[o: o + l] = False
    return bool((h[keep] == GAP).all())


def test_valid_streams_in_one_launch(codec):
    cases = C.valid()
    streams = [v[0] for v in cases.values()] + [b""]
    plains = [v[1] for v in cases.values()] + [b""]
    st, lens, h, off = _decode(codec, streams, [len(p) for p in plains])
    for k, name in enumerate(list(cases) + ["empty"]):
        assert st[k] == R.OK, (name, R.NAMES.get(int(st[k]), st[k]))
        assert lens[k] == len(plains[k]), name
        got = h[off[k]: off[k] + lens[k]].tobytes()
        if got != plains[k]:
            bad = next(i for i, (a, b) in enumerate(zip(got, plains[k])) if a != b)
            raise AssertionError("%s: first difference at byte %d of %d" % (name, bad, len(got)))
    assert _untouched_outside(h, off, lens)


@functools.lru_cache(maxsize=None)
def _malformed():
    """-> [(name, stream, dst_cap, the reference's status, gzip.decompress's bytes or None)]"""
    rows = [("flip%d" % k, s, cap) for k, (s, cap) in enumerate(C.flips())]
    rows += [("cut%d" % k, s, cap) for k, (s, cap) in enumerate(C.truncations())]
    rows += [(name, s, cap) for name, (s, cap, _) in C.hand_built().items()]
    return [(name, s, cap, R.inflate(s, cap=cap)[0], C.gzip_accepts(s)[1]) for name, s, cap in rows]


def test_malformed_streams_in_one_launch(codec):
    rows = _malformed()
    assert len(rows) > 6000
    st, lens, h, off = _decode(codec, [r[1] for r in rows], [r[2] for r in rows])
    hand = C.hand_built()
    wrong = [(name, R.NAMES.get(int(st[k]), int(st[k])), R.NAMES[want]) for k, (name, _, _, want, _) in enumerate(rows) if st[k] != want]
    assert not wrong, (len(wrong), wrong[:10])
    for k, (name, s, cap, want, plain) in enumerate(rows):
        if name in ("two_members", "one_byte_over"):       # gzip.decompress concatenates members; it knows no capacity
            assert plain is not None and st[k] != R.OK
            continue
        assert (st[k] == R.OK) == (plain is not None), name       # OK exactly where gzip.decompress returns
        if plain is not None:
            assert h[off[k]: off[k] + lens[k]].tobytes() == plain, name
        if name in hand:
            assert st[k] == hand[name][2], name
        assert 0 <= lens[k] <= cap, name
    assert _untouched_outside(h, off, [r[2] for r in rows])       # nothing outside the slots, whatever the stream


def test_caller_buffer_contract(codec):
    """dst is an Arena of exactly the summed slots between guards; OK, E_OVERRUN and E_OFFSET streams side by side."""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    v, hb = C.valid(), C.hand_built()
    far, plain = hb["distance_past_output"][0], hb["one_byte_over"][0]
    items = [(v["fixed"][0], 3000, R.OK), (plain, hb["one_byte_over"][1], R.E_OVERRUN), (v["golden_ref_idx_sequence"][0], 12134, R.OK),
             (far, 4, R.E_OFFSET), (v["far_32768"][0], 40000, R.OK), (v["far_32768"][0], 33000, R.E_OVERRUN), (v["file_name"][0], 234, R.OK),
             (v["golden_zlib_contour_map"][0], 15999, R.E_OVERRUN), (b"", 1, R.OK), (v["dynamic_blocks"][0], 3000, R.OK)]
    caps = np.array([c for _, c, _ in items], np.int64)
    off = np.zeros(len(items), np.int64)
    off[1:] = np.cumsum(caps)[:-1]
    assert (off & 1).any()
    arena = BA.Arena(int(caps.sum()), device=dev)
    buf, addr, lens = _sources([s for s, _, _ in items], dev)
    meta = torch.from_numpy(np.stack([addr, lens, off, caps])).to(dev)

    def run(fill):
        arena.raw.fill_(BA.GUARD_BYTE)
        arena.view.fill_(fill)
        from rpcc_amd import _inflate_lib as L
        from rpcc_amd._lib import ptr, stream
        dst_len = BA.filled((len(items),), torch.int64, dev, fill)
        status = BA.filled((len(items),), torch.int32, dev, fill)
        L.check(L.lib().rpcc_inflate_decode(ptr(meta[0]), ptr(meta[1]), len(items), ptr(arena.view), ptr(meta[2]), ptr(meta[3]), ptr(dst_len),
                                            ptr(status), stream()))
        torch.cuda.synchronize()
        assert arena.check_guards() is None, arena.check_guards()
        return {"dst": arena.view.clone(), "dst_len": dst_len, "status": status}

    outs = {}
    holes = BA.unwritten(run, outs)
    assert not holes["dst_len"].any() and not holes["status"].any()        # written for every stream
    st, got = outs["status"].cpu().numpy(), outs["dst_len"].cpu().numpy()
    assert st.tolist() == [w for _, _, w in items]
    hole = holes["dst"].cpu().numpy()
    for k, (s, cap, want) in enumerate(items):
        slot = hole[off[k]: off[k] + cap]
        assert 0 <= got[k] <= cap, k
        if want == R.OK:
            assert not slot[: got[k]].any() and slot[got[k]:].all(), k     # exactly dst_len bytes written
            assert got[k] == len(gzip.decompress(s)), k
        else:
            assert slot[got[k]:].all(), k                                   # nothing past the count produced, so nothing past the slot


def _example_arrays():
    return {k: np.ascontiguousarray(a) for k, a in C.deflate_cases.golden_arrays().items() if k != "zeros"}


def test_basic_compressor_device_entropy_decodes(codec):
    from rpcc_amd import compress_utils as cu
    bc = cu.BasicCompressor(method_name="deflate", device_entropy=True)
    assert bc.batch_decoder() is codec.decompress_many
    d = _example_arrays()
    want = {k: a.tobytes() for k, a in d.items()}
    blobs = bc.compress_dict(d)
    assert bc.decompress_dict(blobs) == want
    assert list(bc.decompress_dict(blobs)) == list(blobs)
    a = np.arange(5000, dtype=np.int16) % 37
    assert bc.decompress(gzip.compress(a)) == a.tobytes()              # any deflate encoder's member
    assert bc.decompress(gzip.compress(a) + bytes(5)) == a.tobytes()   # zero padding, as gzip.decompress reads it
    assert bc.decompress(gzip.compress(b"")) == b"" and bc.decompress(b"") == b""
    frames = [blobs, {"x": gzip.compress(a, 1), "y": gzip.compress(b"")}, {k: blobs[k] for k in list(blobs)[:2]}]
    assert bc.decompress_dicts(frames) == [bc.decompress_dict(f) for f in frames]
    assert bc.decompress_dicts([]) == []
    assert cu.BasicCompressor(method_name="gzip", device_entropy=True).decompress_dict(blobs) == want
    bad = bytearray(blobs["idx_sequence"])
    bad[len(bad) // 2] ^= 0x10
    with pytest.raises(ValueError, match=r"gzip stream 1: .*\(status -\d+\)"):
        bc.decompress_dict({"contour_map": blobs["contour_map"], "idx_sequence": bytes(bad)})
    lying = bytearray(gzip.compress(a))
    lying[-4:] = (len(a.tobytes()) - 1).to_bytes(4, "little")
    st, outs = codec.decode_many([bytes(lying), gzip.compress(a)])
    # (the stated size's high bytes are zero, so the member might as well end earlier, with zero bytes behind it: it is decoded once more
    # with the largest size its last bytes can mean, and is then too long for the size it states)
    assert st.tolist() == [R.E_SIZE, R.OK] and outs == [None, a.tobytes()]
    assert codec.size_fields(np.frombuffer(bytes(lying), np.uint8))[0] == len(a.tobytes()) - 1
    lying[-4:] = (len(a.tobytes()) + 1).to_bytes(4, "little")
    assert codec.decode_many([bytes(lying)])[0].tolist() == [R.E_SIZE]


def _example_bin(tmp_path):
    z = np.load(os.path.join(HERE, "golden", "example_64E.npz"))
    src = tmp_path / "frame.bin"
    np.concatenate((z["xyz"], np.zeros((z["xyz"].shape[0], 1), np.float32)), 1).astype(np.float32).tofile(src)
    return src


def test_compress_decompress_tools(codec, tmp_path, monkeypatch):
    """tools/compress.py then tools/decompress.py with --basic_compressor deflate --device_entropy: the same reconstruction as
    tools/decompress.py without the flag, whose arrays gzip.decompress reads; with the flag they go through inflate_codec."""
    from rpcc_amd.tools import compress as tc
    from rpcc_amd.tools import decompress as td
    src, out = _example_bin(tmp_path), tmp_path / "frame.rpcc"
    base = ["--lidar", "Velodyne64E", "--basic_compressor", "deflate"]
    tc.compress(tc.make_parser().parse_args(["--input", str(src), "--output", str(out), "--device_entropy"] + base))
    calls = []
    monkeypatch.setattr(codec, "decode_many", lambda blobs, device=None, f=codec.decode_many: calls.append(len(blobs)) or f(blobs, device))
    recs = {}
    for flag in ([], ["--device_entropy"]):
        rec = tmp_path / ("rec%d.npy" % len(flag))
        td.decompress(td.make_parser().parse_args(["--input", str(out), "--output", str(rec)] + base + flag))
        recs[len(flag)] = np.load(rec)
        assert calls == ([] if not flag else [4])       # one call for the frame's four arrays
    assert recs[0].shape[0] > 10000 and np.array_equal(recs[0], recs[1])


def test_decompress_datalist_tool(codec, tmp_path, monkeypatch):
    """tools/decompress_datalist.py over three .rpcc files, in chunks of two: the same .bin bytes with and without --device_entropy."""
    from oracle import oracle as orc
    from rpcc_amd import synth
    from rpcc_amd.tools import compress as tc
    from rpcc_amd.tools import decompress_datalist as tdl
    gd = orc.GEOMS["VelodyneVLP16"]
    base = ["--lidar", "VelodyneVLP16", "--basic_compressor", "deflate"]
    names = []
    for k in range(3):
        f = synth.make_frame(60 + k, gd["H"], gd["W"], vmax_deg=gd["vmax_deg"], vmin_deg=gd["vmin_deg"]).numpy()
        src, out = tmp_path / ("sweep%d.bin" % k), tmp_path / ("packed%d.rpcc" % k)
        np.concatenate((f, np.zeros((f.shape[0], 1), np.float32)), 1).astype(np.float32).tofile(src)
        tc.compress(tc.make_parser().parse_args(["--input", str(src), "--output", str(out), "--device_entropy"] + base))
        names.append(str(out))
    lst = tmp_path / "list.txt"
    lst.write_text("\n".join(names) + "\n")
    calls = []
    monkeypatch.setattr(codec, "decode_many", lambda blobs, device=None, f=codec.decode_many: calls.append(len(blobs)) or f(blobs, device))
    monkeypatch.setattr(tdl, "CHUNK", 2)
    files = {}
    for flag in ([], ["--device_entropy"]):
        od = tmp_path / ("out%d" % len(flag))
        tdl.decompress(tc.make_parser(datalist=True).parse_args(["--datalist", str(lst), "--output_dir", str(od)] + base + flag))
        files[len(flag)] = {os.path.basename(f): open(os.path.join(d, f), "rb").read() for d, _, fs in os.walk(od) for f in fs}
    assert calls == [8, 4]                               # chunks of two frames and of one, four arrays each
    assert sorted(files[0]) == ["packed%d.bin" % k for k in range(3)] and files[0] == files[1]
    assert len(set(files[0].values())) == 3 and all(len(v) > 10000 for v in files[0].values())
