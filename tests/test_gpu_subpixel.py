"""-m gpu: the subpixel kernels against tests/subpixel_ref.py, bit for bit, on every case of tests/subpixel_cases.py (payload bytes, nbytes,
orphans, codes, the decoded points and status with uint8 and uint16 label maps; `past_the_grid` takes the code pass's grid-stride loop
through a second trip, tests/subpixel_grid_caps.py), each refusal with its neighbours untouched, the caller-buffer contract, and the
channel end to end: the tools on the example rows, BatchCompressor against the per-frame path with three back-ends, with and without
intensity, behind the radius filter, DBSCAN, NCLT records and the streaming loader."""
import os
import re
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import buffer_arena as BA  # noqa: E402
import intensity_cases as IC  # noqa: E402
import subpixel_cases as SC  # noqa: E402
import subpixel_ref as S  # noqa: E402

_CASE, _MEMO = {}, {}


def ref(name, bits):
    """The case's batch with the reference's results per frame: the owner pass once per distinct frame, the codes once per bits."""
    if name not in _CASE:
        _CASE[name] = SC.CASES[name]()
    batch = _CASE[name]
    return dict(batch, bits=bits, ref=S.encode_frames(batch["frames"], batch["g"], bits, _MEMO.setdefault(name, {})))


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available()
    import __graft_entry__ as ge
    ge.build()
    from rpcc_amd import _lib, compress_utils, ops
    return dict(torch=torch, lib=_lib, ops=ops, cu=compress_utils, dev=torch.device("cuda:0"))


def _upload(env, batch):
    """-> (geom, rows, offsets, ri): with batch["pad"] the frames stand between rows that belong to no frame (offsets[0] > 0, rows behind
    offsets[B]); the range images are made of the frames' own rows."""
    torch, ops, g = env["torch"], env["ops"], batch["g"]
    geom = ops.make_geom(g.H, g.W, g.horizontal_FOV, g.vertical_max, g.vertical_min)
    offs = IC.offsets(batch["frames"])
    body = np.concatenate(batch["frames"])
    front, back = batch["pad"] if batch.get("pad") else (np.zeros((0, 4), np.float32),) * 2
    rows = torch.from_numpy(np.concatenate([front, body, back]).astype(np.float32)).to(env["dev"])
    lo = front.shape[0]
    ri = ops.project(rows[lo: lo + body.shape[0]], torch.from_numpy(offs).to(env["dev"]), geom)
    return geom, rows, torch.from_numpy(offs + lo).to(env["dev"]), ri


def _labels(ri, dtype):
    """A label map whose empty pixels are ri's: 1 where ri == 0, else some other label (0, 2, 3 in turn)."""
    torch = __import__("torch")
    other = (torch.arange(ri.numel(), device=ri.device).view(ri.shape) % 3)
    other = torch.where(other == 1, torch.full_like(other, 3), other)
    lab = torch.where(ri != 0, other, torch.ones_like(other))
    return lab.to(torch.uint8) if dtype == "uint8" else lab.to(torch.int16).view(torch.uint16)


def _tables(env, g):
    return env["torch"].from_numpy(S.tables(g)).to(env["dev"])


def _check(env, batch, outs, ri, tag):
    """payload / nbytes / codes / orphans of one encode call against the batch's references; -> the host copies."""
    g, B = batch["g"], len(batch["frames"])
    P = g.H * g.W
    payload, nbytes, codes, orphans = outs
    assert payload.shape == (B, 8 + 2 * P) and codes.shape == (B, g.H, g.W, 2)
    assert orphans.cpu().tolist() == [0] * B, tag
    ph, nh, ch, rh = payload.cpu().numpy(), nbytes.cpu().numpy(), codes.cpu().numpy().reshape(B, P, 2), ri.cpu().numpy().reshape(B, P)
    bad = []
    for b, e in enumerate(batch["ref"]):
        ok = (np.array_equal(rh[b].view(np.uint32), e["ri"].view(np.uint32)) and nh[b] == e["payload"].shape[0]
              and ph[b, : e["payload"].shape[0]].tobytes() == e["payload"].tobytes() and np.array_equal(ch[b], e["codes"]))
        if not ok:
            bad.append(b)
    assert not bad, (tag, "frames", bad[:8])
    return ph, nh


CASES = [("small", b) for b in (1, 2, 3, 4)] + [("round2", b) for b in (1, 2, 3, 4)] + [("example", 3)]


@pytest.mark.parametrize("name,bits", CASES, ids=["%s-%d" % c for c in CASES])
def test_encode_and_decode_equal_the_reference(env, name, bits):
    torch, ops, lib = env["torch"], env["ops"], env["lib"]
    batch = ref(name, bits)
    g, B = batch["g"], len(batch["frames"])
    P = g.H * g.W
    geom, rows, offs, ri = _upload(env, batch)
    outs = ops.subpixel_encode(rows, offs, geom, ri, bits, want_codes=True)
    ph, nh = _check(env, batch, outs, ri, (name, bits))
    plain = ops.subpixel_encode(rows, offs, geom, ri, bits)                       # without `codes`: the pairs go through the scratch
    assert plain[2] is None and torch.equal(plain[1], outs[1])
    for b in range(B):
        assert plain[0][b, : nh[b]].cpu().numpy().tobytes() == ph[b, : nh[b]].tobytes()
    # the way back, with the owners' own ranges and with ranges of the codec's kind (a hundredth off, some of them negative zero)
    tab = _tables(env, g)
    rec = torch.where(ri != 0, ri + 0.01, -torch.zeros_like(ri))
    for r_dev in (ri, rec):
        decs = {}
        for dt in ("uint8", "uint16"):
            pts, st = ops.subpixel_decode(outs[0], outs[1], _labels(ri, dt), r_dev, tab)
            assert st.cpu().tolist() == [lib.STREAM_OK] * B, (name, dt)
            decs[dt] = pts.cpu().numpy()
        assert decs["uint8"].tobytes() == decs["uint16"].tobytes() and decs["uint8"].shape == (B, g.H, g.W, 3)
        rh = r_dev.cpu().numpy().reshape(B, P)
        for b, e in enumerate(batch["ref"]):
            want = S.decode_frame(e["payload"], np.where(e["ri"] != 0, 0, 1), rh[b], g)
            assert decs["uint8"][b].reshape(P, 3).view(np.uint32).tobytes() == want.view(np.uint32).tobytes(), (name, bits, b)
    if batch["hostile"]:
        print(name, bits, "n", [int(n) for n in nh], "hostile rows", batch["hostile"]["n"])


def test_past_the_grid_twice_and_from_a_dirty_scratch(env):
    """B * P pixels past the cap of subpixel_code_kernel (workgroup 0 takes a second trip) into the caller's buffers: a second call gives
    the same bytes, and so does a call whose scratch holds 0xFF or 0x00 everywhere."""
    import subpixel_grid_caps as GC
    torch, ops, dev = env["torch"], env["ops"], env["dev"]
    batch = ref("past_the_grid", 2)
    g, B = batch["g"], len(batch["frames"])
    P = g.H * g.W
    assert GC.code_trips(B * P) == 2
    geom, rows, offs, ri = _upload(env, batch)
    scratch = torch.empty(env["lib"].lib().rpcc_subpixel_scratch_bytes(B, P), dtype=torch.uint8, device=dev)
    outs = dict(payload=torch.empty((B, 8 + 2 * P), dtype=torch.uint8, device=dev), nbytes=torch.empty((B,), dtype=torch.int32, device=dev),
                codes=torch.empty((B, g.H, g.W, 2), dtype=torch.uint8, device=dev), orphans=torch.empty((B,), dtype=torch.int32, device=dev))
    for tag, fill in (("first", None), ("again", None), ("scratch 0xFF", 0xFF), ("scratch 0x00", 0x00)):
        if fill is not None:
            scratch.fill_(fill)
        for t in outs.values():
            t.zero_()
        got = ops.subpixel_encode(rows, offs, geom, ri, 2, want_codes=True, scratch=scratch, **outs)
        _check(env, batch, got, ri, tag)


def _three(env, bits=3):
    g, rng = IC.orc.LidarGeom(**SC.SMALL), np.random.default_rng(11)
    batch = dict(g=g, frames=[IC.cloud(g, 30, rng, cols=np.arange(0, g.W, 2)) for _ in range(3)], pad=None)   # (every other column stays empty)
    geom, rows, offs, ri = _upload(env, batch)
    payload, nbytes, _, _ = env["ops"].subpixel_encode(rows, offs, geom, ri, bits)
    return g, ri, payload, nbytes


def test_refusals_zero_the_middle_frame_only(env):
    """Each refusal in the middle frame of three: status E_SUBPIXEL and zero points there, the other two untouched."""
    torch, ops, lib = env["torch"], env["ops"], env["lib"]
    bits = 3
    g, ri, payload, nbytes = _three(env, bits)
    P = g.H * g.W
    payload[:, 8:][torch.arange(payload.shape[1] - 8, device=payload.device)[None, :] >= (nbytes[:, None] - 8)] = 0x05     # defined bytes behind every payload (valid codes)
    n1 = int(nbytes[1])
    n = (n1 - 8) // 2
    assert 8 < n1 < 8 + 2 * P and n >= 4
    tab = _tables(env, g)

    def damaged(what):
        p, nb = payload.clone(), nbytes.clone()
        if what == "magic":
            p[1, 3] = ord("2")
        elif what == "intensity magic":
            p[1, 2] = ord("I")
        elif what.startswith("bits "):
            p[1, 4] = int(what[5:])
        elif what.startswith("reserved "):
            p[1, int(what[9:])] = 1
        elif what == "one more":
            nb[1] = n1 + 1
        elif what == "two more":
            nb[1] = n1 + 2
        elif what == "two less":
            nb[1] = n1 - 2
        elif what == "no header":
            nb[1] = 7
        elif what == "no trailer":
            nb[1] = 0
        elif what == "negative":
            nb[1] = -3
        elif what == "past the row":
            nb[1] = p.shape[1] + 2
        elif what == "az code L":
            p[1, 8 + 1] = 1 << bits
        elif what == "el code 255":
            p[1, 8 + n + n - 1] = 255
        elif what == "last az code":
            p[1, 8 + n - 1] = 200
        return p, nb

    cases = ("magic", "intensity magic", "bits 0", "bits 5", "bits 255", "reserved 5", "reserved 6", "reserved 7", "one more", "two more", "two less", "no header",
             "no trailer", "negative", "past the row", "az code L", "el code 255", "last az code")
    for dt in ("uint8", "uint16"):
        lab = _labels(ri, dt)
        good, st = ops.subpixel_decode(payload, nbytes, lab, ri, tab)
        assert st.cpu().tolist() == [0, 0, 0] and good[1].any()
        for what in cases:
            p, nb = damaged(what)
            out = BA.filled(good.shape, torch.float32, env["dev"], 0xFF)
            pts, st = ops.subpixel_decode(p, nb, lab, ri, tab, out=out)
            assert st.cpu().tolist() == [lib.STREAM_OK, lib.STREAM_E_SUBPIXEL, lib.STREAM_OK], (dt, what)
            assert not pts[1].view(torch.int32).any(), (dt, what)
            assert torch.equal(pts[0], good[0]) and torch.equal(pts[2], good[2]), (dt, what)
        # fewer bits than the codes were made with: some code is >= L (bits 1: codes up to 7 stand in the planes)
        p = payload.clone()
        p[1, 4] = 1
        assert int(p[1, 8: n1].max()) >= 2
        assert ops.subpixel_decode(p, nbytes, lab, ri, tab)[1].cpu().tolist() == [0, lib.STREAM_E_SUBPIXEL, 0]
    # a label map with another number of non-empty pixels refuses too
    lab = _labels(ri, "uint8").clone()
    empty = torch.nonzero(lab[1].reshape(-1) == 1).flatten()
    lab[1].view(-1)[empty[0]] = 0
    pts, st = ops.subpixel_decode(payload, nbytes, lab, ri, tab)
    assert st.cpu().tolist() == [0, lib.STREAM_E_SUBPIXEL, 0] and not pts[1].any()


@pytest.mark.parametrize("pattern", ("ones", "intmax", "nan", "alt(0,0)", "alt(0,1)", "half(0)", "half(1)"))
def test_buffer_contract(env, pattern):
    """Exact-size buffers between guard bytes, the scratch filled with a hostile pattern: nothing outside 8 + 2n bytes of a payload row or
    outside any buffer is written, every other output byte is, the results do not depend on what the scratch held, and the decoder reads
    nothing past nbytes."""
    torch, ops, dev = env["torch"], env["ops"], env["dev"]
    bits = 4
    for name in ("small", "round2"):
        batch = ref(name, bits)
        g, B = batch["g"], len(batch["frames"])
        P = g.H * g.W
        geom, rows, offs, ri = _upload(env, batch)
        need = env["lib"].lib().rpcc_subpixel_scratch_bytes(B, P)
        arenas = dict(scratch=BA.Arena(need, dev, back=1 << 16), payload=BA.Arena(B * (8 + 2 * P), dev, back=1 << 16), nbytes=BA.Arena(4 * B, dev, back=4096),
                      codes=BA.Arena(2 * B * P, dev, back=1 << 16), orphans=BA.Arena(4 * B, dev, back=4096))

        def run(fill, with_codes=True):
            for k, a in arenas.items():
                a.fill(pattern if k == "scratch" else "zero")
                if k != "scratch":
                    a.view.fill_(fill)
            ops.subpixel_encode(rows, offs, geom, ri, bits, want_codes=with_codes, payload=arenas["payload"].view.view(B, 8 + 2 * P),
                                nbytes=arenas["nbytes"].view.view(torch.int32), codes=arenas["codes"].view.view(B, g.H, g.W, 2),
                                orphans=arenas["orphans"].view.view(torch.int32), scratch=arenas["scratch"].view)
            torch.cuda.synchronize()
            for k, a in arenas.items():
                assert a.check_guards() is None, (name, pattern, k, a.check_guards())
            return {k: a.view.clone() for k, a in arenas.items() if k != "scratch"}

        outs = {}
        holes = BA.unwritten(run, outs)
        nb = outs["nbytes"].view(torch.int32).cpu().numpy()
        want_holes = (np.arange(8 + 2 * P)[None, :] >= nb[:, None]).reshape(-1)
        assert np.array_equal(holes["payload"].cpu().numpy(), want_holes), (name, pattern)
        for k in ("nbytes", "codes", "orphans"):
            assert not holes[k].any(), (name, pattern, k)
        assert not outs["orphans"].view(torch.int32).any()
        for b, e in enumerate(batch["ref"]):
            assert outs["payload"].view(B, 8 + 2 * P)[b, : nb[b]].cpu().numpy().tobytes() == e["payload"].tobytes(), (name, pattern, b)
            assert np.array_equal(outs["codes"].view(B, P, 2)[b].cpu().numpy(), e["codes"]), (name, pattern, b)
        # without `codes` the pairs lie in the scratch: the same payload, and the caller's codes buffer is not touched
        again = run(0x00, with_codes=False)
        assert torch.equal(again["payload"], outs["payload"]) and torch.equal(again["nbytes"], outs["nbytes"]) and not again["codes"].any()
        # the way back: exact-size inputs and output, and nothing past nbytes is read (two fillings of the rows' tails, one result)
        lab, tab = _labels(ri, "uint8"), _tables(env, g)
        res = []
        for fill in (0x00, 0xFF):
            pay = BA.Arena(B * (8 + 2 * P), dev, back=1 << 16)
            pay.view.copy_(outs["payload"])
            pv = pay.view.view(B, 8 + 2 * P)
            pv[torch.from_numpy(want_holes.reshape(B, 8 + 2 * P)).to(dev)] = fill
            out, st = BA.Arena(12 * B * P, dev, back=1 << 16), BA.Arena(4 * B, dev, back=4096)
            out.view.fill_(0xEE)
            ops.subpixel_decode(pv, outs["nbytes"].view(torch.int32), lab, ri, tab, out=out.view.view(torch.float32).view(B, g.H, g.W, 3),
                                status=st.view.view(torch.int32))
            torch.cuda.synchronize()
            assert out.check_guards() is None and st.check_guards() is None and pay.check_guards() is None
            assert not st.view.any()
            res.append(out.view.clone())
        assert torch.equal(res[0], res[1])
        for b, e in enumerate(batch["ref"]):
            got = res[0].view(torch.float32).view(B, P, 3)[b].cpu().numpy()
            assert got.view(np.uint32).tobytes() == S.decode_frame(e["payload"], np.where(e["ri"] != 0, 0, 1), e["ri"], g).view(np.uint32).tobytes()


def test_orphans_are_counted(env):
    """A range image that is not the image of the rows: the pixels no row owns are counted per frame and coded as (0, 0)."""
    torch, ops = env["torch"], env["ops"]
    batch = ref("small", 2)
    g = batch["g"]
    geom, rows, offs, ri = _upload(env, batch)
    ri2 = ri.clone()
    empty = torch.nonzero(ri2[2].reshape(-1) == 0).flatten()
    ri2[2].view(-1)[empty[:3]] = 5.0                       # three pixels nobody projected to
    ri2[0].view(-1)[torch.nonzero(ri2[0].reshape(-1) != 0).flatten()[0]] += 1.0     # and a depth no row has
    _, nbytes, codes, orphans = ops.subpixel_encode(rows, offs, geom, ri2, 2, want_codes=True)
    assert orphans.cpu().tolist() == [1, 0, 3]
    assert int(nbytes[2]) == batch["ref"][2]["payload"].shape[0] + 6 and not codes[2].reshape(-1, 2)[empty[:3]].any()


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
ACC, GEOM, M, SCALE, BITS = 0.02, "VelodyneVLP16", 40, 100.0, 2
BACKENDS = (("bzip2", {}), ("lz4", {}), ("rans", dict(rans_delta=True)))


@pytest.fixture(scope="module")
def e2e(env):
    from rpcc_amd import dataset, pipeline, synth
    from rpcc_amd.tools.decompress import decode_frame
    gd = IC.orc.GEOMS[GEOM]
    g = IC.orc.LidarGeom(**gd)
    rng = np.random.default_rng(21)
    frames = []
    for i in range(3):
        xyz = synth.make_frame(9100 + i, gd["H"], gd["W"], vmax_deg=gd["vmax_deg"], vmin_deg=gd["vmin_deg"]).numpy()
        frames.append(np.ascontiguousarray(np.concatenate([xyz[:, :3], (rng.integers(0, 100, xyz.shape[0]) / np.float32(100))[:, None]], 1), dtype=np.float32))
    T = dataset.build_dataset(lidar_type=GEOM).PCTransformer
    refs = [S.encode_frame(f, g, BITS) for f in frames]
    return dict(env, pl=pipeline, dec=decode_frame, T=T, g=g, frames=frames, refs=refs, cache={})


def _compress(e2e, method, kw, intensity, subpixel, xyz_only=False):
    key = (method, tuple(sorted(kw.items())), intensity, subpixel, xyz_only)
    if key not in e2e["cache"]:
        bc = e2e["pl"].BatchCompressor(e2e["T"], cluster_num=M, accuracy=ACC, basic_compressor=method, seed=4,
                                       intensity_scale=SCALE if intensity else None, subpixel_bits=BITS if subpixel else None, **kw)
        e2e["cache"][key] = bc.compress([f[:, :3] for f in e2e["frames"]] if xyz_only else e2e["frames"])
    return e2e["cache"][key]


@pytest.mark.parametrize("intensity", (False, True), ids=("plain", "intensity"))
@pytest.mark.parametrize("method,kw", BACKENDS, ids=[m + "".join("+" + k for k in kw) for m, kw in BACKENDS])
def test_batch_compressor_equals_the_per_frame_path(e2e, method, kw, intensity):
    cu, T = e2e["cu"], e2e["T"]
    g = e2e["g"]
    with_s, bare = _compress(e2e, method, kw, intensity, True), _compress(e2e, method, kw, intensity, False)
    if not intensity:
        assert _compress(e2e, method, kw, False, True, xyz_only=True) == with_s           # [N,3] frames: a zero fourth column on the host
    bc = cu.BasicCompressor(method_name=method, **kw)
    host = cu.BasicCompressor(method_name=method)
    for b, (blob, base) in enumerate(zip(with_s, bare)):
        assert blob[: len(base)] == base and len(blob) > len(base) + 4, (method, b)        # the bytes before the trailer: the container without it
        cd = cu.unpack_bitstream(blob, intensity=intensity, subpixel=True)
        assert tuple(cd)[-1] == "subpixel" and len(base) + 4 + len(cd["subpixel"]) == len(blob)
        assert bytes(host.decompress(cd["subpixel"])) == e2e["refs"][b]["payload"].tobytes(), (method, b)
        # the per-frame path: the frame's rows against its own range image, through compress_point_cloud's arguments
        plain = cu.unpack_bitstream(base)
        nrows = len(host.decompress(plain["plane_param"])) // 16
        rq, idx_map, sal, plane = cu.decompress_point_cloud(plain, host, nrows, T.H, T.W)
        ri = T.point_cloud_to_range_image(e2e["frames"][b])
        spay, codes = cu.encode_subpixel(T, e2e["frames"][b][:, :3] if b == 1 else e2e["frames"][b], ri, BITS, want_codes=True)
        assert spay.tobytes() == e2e["refs"][b]["payload"].tobytes() and np.array_equal(codes.reshape(-1, 2), e2e["refs"][b]["codes"])
        ipay = cu.encode_intensity(T, e2e["frames"][b], ri, SCALE)[0] if intensity else None
        original, compressed = cu.compress_point_cloud(bc, plane, idx_map, sal, rq, intensity=ipay, subpixel=spay)
        assert ("intensity" in original) == intensity and original["subpixel"].tobytes() == spay.tobytes()
        assert blob == cu.pack_bitstream(compressed), (method, b, "per frame")
        # the way back: the points are the reference's, made of the decoder's own ranges
        rec, pc, seg, *w = e2e["dec"](cd, host, T, M, 2 * ACC, None, True, intensity=intensity, subpixel=True)
        want = S.decode_frame(e2e["refs"][b]["payload"], seg.reshape(-1), rec.reshape(-1), g)
        assert pc.dtype == np.float32 and pc.reshape(-1, 3).view(np.uint32).tobytes() == want.view(np.uint32).tobytes(), (method, b)
        rec0, pc0, seg0 = e2e["dec"](cu.unpack_bitstream(blob), host, T, M, 2 * ACC, None, True)[:3]       # a reader that does not ask: today's result
        assert rec0.tobytes() == rec.tobytes() and seg0.tobytes() == seg.tobytes() and pc0.tobytes() == T.range_image_to_point_cloud(rec).tobytes()
        assert len(w) == (1 if intensity else 0)
        with pytest.raises(ValueError, match="no subpixel trailer"):
            cu.unpack_bitstream(base, intensity=intensity, subpixel=True)
    # a damaged payload: decode_frame refuses by name
    cd = cu.unpack_bitstream(with_s[0], intensity=intensity, subpixel=True)
    raw = bytearray(host.decompress(cd["subpixel"]))
    raw[9] = 200
    with pytest.raises(ValueError, match="subpixel payload: code 200"):
        e2e["dec"](dict(cd, subpixel=host.compress(np.frombuffer(bytes(raw), np.uint8))), host, T, M, 2 * ACC, None, True, intensity=intensity, subpixel=True)


def test_radius_filter_dbscan_and_orphans(e2e):
    from rpcc_amd.outlier import remove_radius_outlier
    cu, T, g = e2e["cu"], e2e["T"], e2e["g"]
    host = cu.BasicCompressor(method_name="bzip2")
    bc = e2e["pl"].BatchCompressor(T, cluster_num=M, accuracy=ACC, basic_compressor="bzip2", seed=4, subpixel_bits=BITS, radius_outlier_removal=(3, 1.0))
    lone = IC.rays(g, [3, 5, 7, 9, 11], [100, 400, 700, 1000, 1300], [150.0] * 5, [.5] * 5)     # five lone points far out: the filter has something to remove
    frames = [np.concatenate([f[:1000], lone, f[1000:]]) for f in e2e["frames"][:2]]
    removed = 0
    for b, blob in enumerate(bc.compress(frames)):
        kept = frames[b][remove_radius_outlier(frames[b], nb_points=3, radius=1.0)[1]]
        removed += frames[b].shape[0] - kept.shape[0]
        want = S.encode_frame(kept, g, BITS)["payload"]
        assert bytes(host.decompress(cu.unpack_bitstream(blob, subpixel=True)["subpixel"])) == want.tobytes(), b
    assert removed > 0
    mk = lambda bits: e2e["pl"].BatchCompressor(T, accuracy=ACC, basic_compressor="bzip2", seed=4, subpixel_bits=bits, intensity_scale=SCALE,
                                                segment_method="DBSCAN", max_labels=1023)
    blob, base = mk(BITS).compress(e2e["frames"][:1])[0], mk(None).compress(e2e["frames"][:1])[0]
    cd = cu.unpack_bitstream(blob, intensity=True, subpixel=True)
    assert blob[: len(base)] == base and bytes(host.decompress(cd["subpixel"])) == e2e["refs"][0]["payload"].tobytes()
    rec, pc, seg, w = e2e["dec"](cd, host, T, None, 2 * ACC, None, True, intensity=True, subpixel=True)
    assert pc.reshape(-1, 3).view(np.uint32).tobytes() == S.decode_frame(e2e["refs"][0]["payload"], seg.reshape(-1), rec.reshape(-1), g).view(np.uint32).tobytes()


def test_nclt_records_and_streaming_loader(e2e, tmp_path):
    from rpcc_amd import records
    from rpcc_amd.loader import StreamingCompressor
    cu, T, g = e2e["cu"], e2e["T"], e2e["g"]
    host = cu.BasicCompressor(method_name="bzip2")
    paths = []
    for i, f in enumerate(e2e["frames"][:2]):
        paths.append(str(tmp_path / ("%d.bin" % i)))
        f.tofile(paths[-1])
    mk = lambda **kw: e2e["pl"].BatchCompressor(T, cluster_num=M, accuracy=ACC, basic_compressor="bzip2", seed=4, subpixel_bits=BITS, **kw)
    got = {}
    sc = StreamingCompressor(mk(intensity_scale=SCALE), batch=2, depth=2, workers=2, ingest="rows")
    assert sc.run([(paths, [0, 1])], sink=lambda k, blobs: got.update({k: blobs})) == 2
    assert got[0] == _compress(e2e, "bzip2", {}, True, True)[:2]
    with pytest.raises(ValueError, match='ingest="rows"'):
        StreamingCompressor(mk(), batch=2, depth=2, workers=2, ingest="xyz")
    # NCLT records: the rows the device unpacks are the rows of records.unpack_host
    rng = np.random.default_rng(5)
    rec = np.zeros((4000, records.RECORD_BYTES), np.uint8)
    rec[:, :6] = rng.integers(0, 256, (4000, 6))
    rec[:, 1:6:2] = rng.integers(70, 86, (4000, 3))                # the high bytes: coordinates within ten metres
    rec[:, 6] = rng.integers(0, 256, 4000)
    blob = mk(point_format="nclt").compress([rec])[0]
    want = S.encode_frame(records.unpack_host(rec), g, BITS)["payload"]
    assert bytes(host.decompress(cu.unpack_bitstream(blob, subpixel=True)["subpixel"])) == want.tobytes()


def test_tools_round_trip_on_the_example_rows(env, tmp_path, capsys):
    """tools/compress.py then tools/decompress.py with --subpixel 2 on the example rows: the points written are the reference file's."""
    from rpcc_amd.tools import compress as tc
    from rpcc_amd.tools import decompress as td
    cu = env["cu"]
    batch = ref("example", 2)
    g, rows, e = batch["g"], batch["frames"][0], batch["ref"][0]
    src, out, rec_f = tmp_path / "frame.bin", tmp_path / "frame.rpcc", tmp_path / "rec.bin"
    rows.tofile(src)
    base = ["--lidar", "Velodyne64E", "--basic_compressor", "bzip2"]
    capsys.readouterr()
    tc.compress(tc.make_parser().parse_args(["--input", str(src), "--output", str(out), "--eval", "--subpixel", "2"] + base))
    text = capsys.readouterr().out
    assert "(subpixel: the refined points against the original points)" in text
    refined = float(re.search(r"^    Chamfer Distance \(mean\): +([0-9.eE+-]+)", text, re.M).group(1))
    td.decompress(td.make_parser().parse_args(["--input", str(out), "--output", str(rec_f), "--subpixel", "2"] + base))
    got = np.fromfile(rec_f, np.float32).reshape(-1, 4)
    td.decompress(td.make_parser().parse_args(["--input", str(out), "--output", str(tmp_path / "bare_flag.bin"), "--subpixel"] + base))   # the bare flag: the same file
    assert np.fromfile(tmp_path / "bare_flag.bin", np.float32).tobytes() == got.tobytes()
    td.decompress(td.make_parser().parse_args(["--input", str(out), "--output", str(tmp_path / "zero.bin"), "--subpixel", "0"] + base))   # any value: on
    assert np.fromfile(tmp_path / "zero.bin", np.float32).tobytes() == got.tobytes()
    host = cu.BasicCompressor(method_name="bzip2")
    cd = cu.read_compressed_bitstream(str(out), subpixel=True)
    assert bytes(host.decompress(cd["subpixel"])) == e["payload"].tobytes()
    T = __import__("rpcc_amd.dataset", fromlist=["x"]).build_dataset(lidar_type="Velodyne64E").PCTransformer
    _, accuracy, segment_cfg, _, _, uniform = tc.resolve_cfg(tc.make_parser().parse_args(base))
    assert uniform
    rec, pc, seg = td.decode_frame(cd, host, T, segment_cfg["cluster_num"], accuracy, None, True, subpixel=True)
    want = S.decode_frame(e["payload"], seg.reshape(-1), rec.reshape(-1), g)
    assert pc.reshape(-1, 3).view(np.uint32).tobytes() == want.view(np.uint32).tobytes()
    keep = want.sum(-1) != 0
    assert np.array_equal(got[:, :3].view(np.uint32), want[keep].view(np.uint32)) and not got[:, 3].any()
    # without the flag: today's file and today's container
    td.decompress(td.make_parser().parse_args(["--input", str(out), "--output", str(tmp_path / "plain.bin")] + base))
    plain = np.fromfile(tmp_path / "plain.bin", np.float32).reshape(-1, 4)
    centre = T.range_image_to_point_cloud(rec).reshape(-1, 3)
    assert np.array_equal(plain[:, :3], centre[centre.sum(-1) != 0])
    bare = tmp_path / "bare.rpcc"
    tc.compress(tc.make_parser().parse_args(["--input", str(src), "--output", str(bare)] + base))
    assert open(out, "rb").read()[: os.path.getsize(bare)] == open(bare, "rb").read()
    with pytest.raises(ValueError, match="no subpixel trailer"):
        td.decompress(td.make_parser().parse_args(["--input", str(bare), "--output", str(rec_f), "--subpixel"] + base))
    # the refined points are nearer to the original points than the pixel centres are
    from rpcc_amd.evaluate_metrics import calc_chamfer_distance
    off = calc_chamfer_distance(rows[:, :3], centre, out=False)["mean"]
    print("Chamfer against the original points: pixel centres", off, "--subpixel 2", refined)
    assert refined < off
