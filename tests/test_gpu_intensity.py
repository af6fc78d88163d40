"""-m gpu: the intensity kernels against tests/intensity_ref.py on every case of tests/intensity_cases.py (payload bytes, nbytes, image,
orphans == 0, the way back with uint8 and uint16 label maps; `past_the_grid` takes every grid-stride loop past its cap, tests/grid_caps.py),
the four refusals, the caller-buffer contract, and the channel end to end
at 16 x 1800 through the per-frame path, BatchCompressor / BatchDecompressor with every back-end, the radius filter, DBSCAN, uint16 labels,
the streaming loader and the tools."""
import os
import re
import struct
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import buffer_arena as BA  # noqa: E402
import gzip_compare as GZ  # noqa: E402
import intensity_cases as IC  # noqa: E402
import intensity_ref as R  # noqa: E402

_REF = {}


def ref(name):
    """The case's batches with the reference's results per frame, computed once and shared."""
    if name not in _REF:
        _REF[name] = [dict(b, ref=R.encode_frames(b["frames"], b["g"], b["scale"])) for b in IC.CASES[name]()]     # (once per distinct frame)
    return _REF[name]


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available()
    import __graft_entry__ as ge
    ge.build()
    from rpcc_amd import _lib, compress_utils, ops
    return dict(torch=torch, lib=_lib, ops=ops, cu=compress_utils, dev=torch.device("cuda:0"))


def _upload(env, batch):
    torch, ops, g = env["torch"], env["ops"], batch["g"]
    geom = ops.make_geom(g.H, g.W, g.horizontal_FOV, g.vertical_max, g.vertical_min)
    rows = torch.from_numpy(np.concatenate(batch["frames"])).to(env["dev"])
    offs = torch.from_numpy(IC.offsets(batch["frames"])).to(env["dev"])
    return geom, rows, offs


def _labels(ri, dtype):
    """A label map whose empty pixels are ri's: 1 where ri == 0, else some other label (0, 2, 3 in turn)."""
    torch = __import__("torch")
    other = (torch.arange(ri.numel(), device=ri.device).view(ri.shape) % 3)
    other = torch.where(other == 1, torch.full_like(other, 3), other)
    lab = torch.where(ri != 0, other, torch.ones_like(other))
    return lab.to(torch.uint8) if dtype == "uint8" else lab.to(torch.int16).view(torch.uint16)


@pytest.mark.parametrize("name", list(IC.CASES))
def test_encode_and_decode_equal_the_reference(env, name):
    torch, ops, lib = env["torch"], env["ops"], env["lib"]
    for batch in ref(name):
        g, scale, B = batch["g"], batch["scale"], len(batch["frames"])
        P = g.H * g.W
        geom, rows, offs = _upload(env, batch)
        ri = ops.project(rows, offs, geom)
        ri_atomic = ops.project(rows, offs, geom, atomic_path=True)
        own = torch.empty_like(ri)
        payload, nbytes, image, orphans = ops.intensity_encode(rows, offs, geom, ri, scale, want_image=True, owner_intensity=own)
        p2, n2, im2, o2 = ops.intensity_encode(rows, offs, geom, ri_atomic, scale, want_image=True)
        assert payload.shape == (B, 8 + P) and image.shape == (B, g.H, g.W)
        assert orphans.cpu().tolist() == [0] * B and o2.cpu().tolist() == [0] * B
        ph, nh, ih, oh, rh = payload.cpu().numpy(), nbytes.cpu().numpy(), image.cpu().numpy(), own.cpu().numpy(), ri.cpu().numpy()
        p2h = p2.cpu().numpy()
        assert np.array_equal(nh, n2.cpu().numpy()) and np.array_equal(ih, im2.cpu().numpy())
        decs = {}
        for dt in ("uint8", "uint16"):
            w, st = ops.intensity_decode(payload, nbytes, _labels(ri, dt))
            assert st.cpu().tolist() == [lib.STREAM_OK] * B, (name, dt)
            decs[dt] = w.cpu().numpy()
        assert decs["uint8"].tobytes() == decs["uint16"].tobytes()
        for b, (f, e) in enumerate(zip(batch["frames"], batch["ref"])):
            assert np.array_equal(rh[b].reshape(-1).view(np.uint32), e["ri"].view(np.uint32)), (name, b)
            assert nh[b] == e["payload"].shape[0], (name, b, nh[b], e["payload"].shape[0])
            assert ph[b, : nh[b]].tobytes() == e["payload"].tobytes(), (name, b)
            assert p2h[b, : nh[b]].tobytes() == e["payload"].tobytes(), (name, b)
            assert np.array_equal(ih[b].reshape(-1), e["image"]), (name, b)
            set_ = e["ri"] != 0
            w_own = f[e["own"][set_], 3]
            assert np.array_equal(oh[b].reshape(-1)[set_].view(np.uint32), w_own.view(np.uint32)) and not oh[b].reshape(-1)[~set_].any()
            back = decs["uint8"][b].reshape(-1)
            assert np.array_equal(back.view(np.uint32), R.decode_frame(e["payload"], np.where(set_, 0, 1)).view(np.uint32)), (name, b)
            # within half a step of the owner's value wherever the quantiser does not clamp; the products and the quotient are fp32: an ulp each
            with np.errstate(all="ignore"):
                t = w_own * np.float32(scale)
                inside = np.isfinite(t) & (t >= 0) & (t <= 255)
            err = np.abs(back[set_][inside].astype(np.float64) - w_own[inside].astype(np.float64))
            tol = 0.5 / scale + 2.0 ** -23 * np.maximum(1.0, np.abs(w_own[inside].astype(np.float64)))
            if b < 4 or "distinct" not in batch:     # (a batch that repeats four frames: one line per distinct frame)
                print(name, b, "n", int(set_.sum()), "max err", float(err.max()) if err.size else 0.0, "bound", 0.5 / scale)
            assert np.all(err <= tol), (name, b, float(err.max()))
            if name == "example" or (name == "rounding" and scale == 100):
                assert np.array_equal(back[set_].view(np.uint32), w_own.view(np.uint32)), (name, b)     # bit-equal to the input column
        if name == "example":
            z = np.load(os.path.join(HERE, "golden", "intensity_example_64E.npz"))
            assert ph[0, : nh[0]].tobytes() == z["payload"].tobytes()


def _expected_rows(batch):
    """(payload rows u8 [B, 8+P] with zeros behind nbytes, nbytes i32 [B], image u8 [B,P]) of a batch, from its references."""
    P = batch["g"].H * batch["g"].W
    rows = np.zeros((len(batch["ref"]), 8 + P), np.uint8)
    for b, e in enumerate(batch["ref"]):
        rows[b, : e["payload"].shape[0]] = e["payload"]
    return rows, np.array([e["payload"].shape[0] for e in batch["ref"]], np.int32), np.stack([e["image"] for e in batch["ref"]])


def test_past_the_grid_twice_and_from_a_dirty_scratch(env):
    """The batch past the grid caps (two trips of the fill kernel and the owner pass, three of the fix-up pass) into the caller's buffers: a
    second call gives the same bytes, and so does a call whose scratch holds 0xFF everywhere -- the upper half of the owner and lastz
    planes is what the fill kernel's second trip initialises."""
    import grid_caps as GC
    torch, ops, dev = env["torch"], env["ops"], env["dev"]
    batch = ref("past_the_grid")[0]
    g, B = batch["g"], len(batch["frames"])
    P = g.H * g.W
    geom, rows, offs = _upload(env, batch)
    total = rows.shape[0]
    assert B * P > GC.INT_FILL_CAP * GC.INT_FILL_THREADS and total > GC.INT_OWNER_CAP * GC.INT_THREADS and total > 2 * GC.INT_FIXUP_CAP * GC.INT_THREADS
    ri = ops.project(rows, offs, geom)
    want_rows, want_n, want_image = _expected_rows(batch)
    scratch = torch.empty(env["lib"].lib().rpcc_intensity_scratch_bytes(B, P), dtype=torch.uint8, device=dev)
    outs = dict(payload=torch.empty((B, 8 + P), dtype=torch.uint8, device=dev), nbytes=torch.empty((B,), dtype=torch.int32, device=dev),
                image=torch.empty((B, g.H, g.W), dtype=torch.uint8, device=dev), orphans=torch.empty((B,), dtype=torch.int32, device=dev))
    for tag, fill in (("first", None), ("again", None), ("scratch 0xFF", 0xFF), ("scratch 0x00", 0x00)):
        if fill is not None:
            scratch.fill_(fill)
        for t in outs.values():
            t.zero_()
        ops.intensity_encode(rows, offs, geom, ri, batch["scale"], want_image=True, scratch=scratch, **outs)
        assert outs["orphans"].cpu().tolist() == [0] * B, tag
        assert np.array_equal(outs["nbytes"].cpu().numpy(), want_n), tag
        got = outs["payload"].cpu().numpy()
        bad = np.flatnonzero((got != want_rows).any(1))
        assert bad.size == 0, (tag, "frames", bad[:8].tolist(), "of kinds", batch["which"][bad[:8]].tolist())
        assert np.array_equal(outs["image"].cpu().numpy().reshape(B, P), want_image), tag
    # for the record: what the screened path really sends to the queue in the two chunks of the first workgroup whose drain leaves a remainder
    queued = np.concatenate([(e["pix"] < 0) | (e["pix"] % g.W == 0) | (e["d"] == 0) for e in batch["ref"]])
    maybe = np.concatenate([~batch["aimed_fast"][k] for k in batch["which"]])
    w = int(GC.queue_facts(queued, maybe, total, GC.INT_THREADS, GC.INT_OWNER_CAP, GC.INT_THREADS)["remainder"][0])
    for r in (0, 1):
        a, b = GC.owner_rows(total, w, r)
        sure, bad, slow = ops.project_fastpath_check(rows[a:b, :3].contiguous(), geom)[:3]
        print("workgroup %d trip %d: rows %d .. %d, %d queued by rule, %d sent to the exact sequence" % (w, r, a, b, int(queued[a:b].sum()), slow))
        assert bad == 0 and slow >= int(queued[a:b].sum())


def test_past_the_grid_through_the_batch_compressor(env):
    """The same 247 frames of rows through BatchCompressor(intensity_scale=255): every container's intensity trailer decodes to the
    reference's payload of its frame (the geometry columns are other tests' matter)."""
    from rpcc_amd.pipeline import BatchCompressor
    from rpcc_amd.transformer import PCTransformer
    cu = env["cu"]
    batch = ref("past_the_grid")[0]
    T = PCTransformer(dict(HORIZONTAL_FOV=IC.PAST_GEOM["hfov_deg"], VERTICAL_ANGLE_MAX=IC.PAST_GEOM["vmax_deg"], VERTICAL_ANGLE_MIN=IC.PAST_GEOM["vmin_deg"],
                           RANGE_IMAGE_HEIGHT=IC.PAST_GEOM["H"], RANGE_IMAGE_WIDTH=IC.PAST_GEOM["W"]), device=env["dev"])
    bc = BatchCompressor(T, cluster_num=10, accuracy=0.02, basic_compressor="bzip2", seed=4, intensity_scale=batch["scale"])
    blobs = bc.compress(batch["frames"])
    host = cu.BasicCompressor(method_name="bzip2")
    assert len(blobs) == len(batch["frames"])
    for b, (blob, e) in enumerate(zip(blobs, batch["ref"])):
        span = cu.intensity_trailer_span(blob)
        assert span is not None, b
        assert bytes(host.decompress(blob[span[0]: span[1]])) == e["payload"].tobytes(), (b, int(batch["which"][b]))


def test_refusals_zero_the_middle_frame_only(env):
    """Each refusal in the middle frame of three: status E_INTENSITY and a zero row there, the other two untouched."""
    torch, ops, lib = env["torch"], env["ops"], env["lib"]
    g, rng = IC.orc.LidarGeom(**IC.TINY), np.random.default_rng(11)
    batch = dict(g=g, frames=[IC.cloud(g, 30, rng, cols=np.arange(0, g.W, 2)) for _ in range(3)], scale=255.0)   # (every other column stays empty)
    geom, rows, offs = _upload(env, batch)
    ri = ops.project(rows, offs, geom)
    payload, nbytes, _, _ = ops.intensity_encode(rows, offs, geom, ri, 255.0)
    payload[:, 8:][torch.arange(payload.shape[1] - 8, device=payload.device)[None, :] >= (nbytes[:, None] - 8)] = 0x5A     # defined bytes behind every payload
    n1 = int(nbytes[1])
    assert 8 < n1 < 8 + g.H * g.W

    def damaged(what):
        p, n = payload.clone(), nbytes.clone()
        if what == "magic":
            p[1, 3] = ord("2")
        elif what in ("scale 0", "scale nan", "scale inf", "scale -1"):
            v = dict(zip(("scale 0", "scale nan", "scale inf", "scale -1"), (0.0, float("nan"), float("inf"), -1.0)))[what]
            p[1, 4:8] = torch.tensor(list(struct.pack("<f", v)), dtype=torch.uint8)
        elif what == "one more":
            n[1] = n1 + 1
        elif what == "one less":
            n[1] = n1 - 1
        elif what == "no header":
            n[1] = 7
        elif what == "no trailer":
            n[1] = 0
        elif what == "negative":
            n[1] = -3
        elif what == "past the row":
            n[1] = p.shape[1] + 1
        return p, n

    for dt in ("uint8", "uint16"):
        lab = _labels(ri, dt)
        good, st = ops.intensity_decode(payload, nbytes, lab)
        assert st.cpu().tolist() == [0, 0, 0] and good[1].any()
        for what in ("magic", "scale 0", "scale nan", "scale inf", "scale -1", "one more", "one less", "no header", "no trailer", "negative", "past the row"):
            p, n = damaged(what)
            out = BA.filled(good.shape, torch.float32, env["dev"], 0xFF)
            w, st = ops.intensity_decode(p, n, lab, out=out)
            assert st.cpu().tolist() == [lib.STREAM_OK, lib.STREAM_E_INTENSITY, lib.STREAM_OK], (dt, what)
            assert not w[1].view(torch.int32).any(), (dt, what)
            assert torch.equal(w[0], good[0]) and torch.equal(w[2], good[2]), (dt, what)
    # a label map with another number of non-empty pixels refuses too
    lab = _labels(ri, "uint8").clone()
    empty = torch.nonzero(lab[1].reshape(-1) == 1).flatten()
    lab[1].view(-1)[empty[0]] = 0
    w, st = ops.intensity_decode(payload, nbytes, lab)
    assert st.cpu().tolist() == [0, lib.STREAM_E_INTENSITY, 0] and not w[1].any()


@pytest.mark.parametrize("pattern", ("ones", "intmax", "nan", "alt(0,0)", "alt(0,1)", "half(0)", "half(1)"))
def test_buffer_contract(env, pattern):
    """Exact-size buffers between guard bytes, the scratch filled with a hostile pattern: nothing outside 8 + n bytes of a payload row or
    outside any buffer is written, every other output byte is, the results do not depend on what the scratch held, and the decoder reads
    nothing past nbytes."""
    torch, ops, dev = env["torch"], env["ops"], env["dev"]
    for name in ("zeros", "frames"):
        batch = ref(name)[0]
        g, B = batch["g"], len(batch["frames"])
        P = g.H * g.W
        geom, rows, offs = _upload(env, batch)
        ri = ops.project(rows, offs, geom)
        need = env["lib"].lib().rpcc_intensity_scratch_bytes(B, P)
        arenas = dict(scratch=BA.Arena(need, dev, back=1 << 16), payload=BA.Arena(B * (8 + P), dev, back=1 << 16), nbytes=BA.Arena(4 * B, dev, back=4096),
                      image=BA.Arena(B * P, dev, back=1 << 16), orphans=BA.Arena(4 * B, dev, back=4096), own=BA.Arena(4 * B * P, dev, back=1 << 16))

        def run(fill):
            for k, a in arenas.items():
                a.fill(pattern if k == "scratch" else "zero")
                if k != "scratch":
                    a.view.fill_(fill)
            ops.intensity_encode(rows, offs, geom, ri, batch["scale"], want_image=True, payload=arenas["payload"].view.view(B, 8 + P),
                                 nbytes=arenas["nbytes"].view.view(torch.int32), image=arenas["image"].view.view(B, g.H, g.W),
                                 orphans=arenas["orphans"].view.view(torch.int32), scratch=arenas["scratch"].view,
                                 owner_intensity=arenas["own"].view.view(torch.float32).view(B, g.H, g.W))
            torch.cuda.synchronize()
            for k, a in arenas.items():
                assert a.check_guards() is None, (name, pattern, k, a.check_guards())
            return {k: a.view.clone() for k, a in arenas.items() if k != "scratch"}

        outs = {}
        holes = BA.unwritten(run, outs)
        nb = outs["nbytes"].view(torch.int32).cpu().numpy()
        want_holes = (np.arange(8 + P)[None, :] >= nb[:, None]).reshape(-1)
        assert np.array_equal(holes["payload"].cpu().numpy(), want_holes), (name, pattern)
        for k in ("nbytes", "image", "orphans", "own"):
            assert not holes[k].any(), (name, pattern, k)
        assert not outs["orphans"].view(torch.int32).any()
        for b, e in enumerate(batch["ref"]):
            assert outs["payload"].view(B, 8 + P)[b, : nb[b]].cpu().numpy().tobytes() == e["payload"].tobytes(), (name, pattern, b)
            assert np.array_equal(outs["image"].view(B, P)[b].cpu().numpy(), e["image"]), (name, pattern, b)
        # the way back: exact-size inputs and output, and nothing past nbytes is read (two fillings of the rows' tails, one result)
        lab = _labels(ri, "uint8")
        res = []
        for fill in (0x00, 0xFF):
            pay = BA.Arena(B * (8 + P), dev, back=1 << 16)
            pay.view.copy_(outs["payload"])
            pv = pay.view.view(B, 8 + P)
            pv[torch.from_numpy(want_holes.reshape(B, 8 + P)).to(dev)] = fill
            out, st = BA.Arena(4 * B * P, dev, back=1 << 16), BA.Arena(4 * B, dev, back=4096)
            out.view.fill_(0xEE)
            ops.intensity_decode(pv, outs["nbytes"].view(torch.int32), lab, out=out.view.view(torch.float32).view(B, g.H, g.W), status=st.view.view(torch.int32))
            torch.cuda.synchronize()
            assert out.check_guards() is None and st.check_guards() is None and pay.check_guards() is None
            assert not st.view.any()
            res.append(out.view.clone())
        assert torch.equal(res[0], res[1])
        for b, e in enumerate(batch["ref"]):
            got = res[0].view(torch.float32).view(B, P)[b].cpu().numpy()
            assert np.array_equal(got.view(np.uint32), R.decode_frame(e["payload"], np.where(e["ri"] != 0, 0, 1)).view(np.uint32))


# ---- end to end at 16 x 1800 ---------------------------------------------------------------------------------------------------------
ACC, GEOM, M, SCALE = 0.02, "VelodyneVLP16", 40, 100.0
BACKENDS = (("lz4", {}), ("bzip2", {}), ("gzip", {}), ("deflate", {}), ("rans", {}), ("rans", dict(rans_delta=True)),
            ("deflate", dict(device_entropy=True)), ("bzip2", dict(device_bzip2=True)))


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
    refs = [R.encode_frame(f, g, SCALE) for f in frames]
    want = [np.where(e["ri"] != 0, e["image"].astype(np.float32) / np.float32(SCALE), np.float32(0)).reshape(g.H, g.W) for e in refs]
    return dict(env, pl=pipeline, dec=decode_frame, T=T, g=g, frames=frames, refs=refs, want=want, cache={})


def _compress(e2e, method, kw, intensity):
    key = (method, tuple(sorted(kw.items())), intensity)
    if key not in e2e["cache"]:
        bc = e2e["pl"].BatchCompressor(e2e["T"], cluster_num=M, accuracy=ACC, basic_compressor=method, seed=4,
                                       intensity_scale=SCALE if intensity else None, **kw)
        e2e["cache"][key] = bc.compress(e2e["frames"] if intensity else [f[:, :3] for f in e2e["frames"]])
    return e2e["cache"][key]


@pytest.mark.parametrize("method,kw", BACKENDS, ids=[m + "".join("+" + k for k in kw) for m, kw in BACKENDS])
def test_end_to_end(e2e, method, kw):
    cu, T, lib = e2e["cu"], e2e["T"], e2e["lib"]
    with_w, plain = _compress(e2e, method, kw, True), _compress(e2e, method, kw, False)
    bc = cu.BasicCompressor(method_name=method, **kw)
    host = cu.BasicCompressor(method_name=method)
    bd = e2e["pl"].BatchDecompressor(T, M, 2 * ACC, basic_compressor=method, intensity=True)
    batch = bd.decompress(with_w)
    geometry = e2e["pl"].BatchDecompressor(T, M, 2 * ACC, basic_compressor=method).decompress(with_w)

    def same(x, y, tag):
        """Two containers byte for byte; where separate gzip.compress calls on the host wrote them, but for the members' MTIME bytes."""
        if method in ("gzip", "deflate") and not kw:
            GZ.assert_equal_but_mtime(x, y, tag)
        else:
            assert x == y, tag

    for b, (blob, bare) in enumerate(zip(with_w, plain)):
        same(blob[: len(bare)], bare, (method, b, "prefix"))                                    # the bytes before the trailer: the container without it
        assert len(blob) > len(bare) + 4, (method, b)
        span = cu.intensity_trailer_span(blob)
        assert span is not None and span[0] == len(bare) + 4
        assert bytes(host.decompress(blob[span[0]: span[1]])) == e2e["refs"][b]["payload"].tobytes(), (method, b)
        # the per-frame path: the frame's rows against its own range image, through compress_point_cloud's argument
        cd = cu.unpack_bitstream(bare)
        rows = len(host.decompress(cd["plane_param"])) // 16
        rq, idx_map, sal, plane = cu.decompress_point_cloud(cd, host, rows, T.H, T.W)
        pay, _ = cu.encode_intensity(T, e2e["frames"][b], T.point_cloud_to_range_image(e2e["frames"][b]), SCALE)
        assert pay.tobytes() == e2e["refs"][b]["payload"].tobytes()
        _, compressed = cu.compress_point_cloud(bc, plane, idx_map, sal, rq, intensity=pay)
        same(blob, cu.pack_bitstream(compressed), (method, b, "per frame"))
        # the way back, per frame and batched
        rec, pc, seg, w = e2e["dec"](cu.unpack_bitstream(blob, intensity=True), host, T, M, 2 * ACC, None, True, intensity=True)
        assert w.dtype == np.float32 and w.tobytes() == e2e["want"][b].tobytes(), (method, b)
        assert np.array_equal(seg == 1, e2e["refs"][b]["ri"].reshape(T.H, T.W) == 0)
        for name, x, y in zip(("rec", "pc", "seg", "intensity"), batch[b], (rec, pc, seg, w)):
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), (method, b, name)
        assert len(geometry[b]) == 3 and geometry[b][0].tobytes() == rec.tobytes()               # a caller that does not ask: today's result
        with pytest.raises(ValueError, match="no intensity trailer"):
            cu.unpack_bitstream(bare, intensity=True)
    # frames with and without the trailer in one batch: E_INTENSITY for exactly the frames without
    mixed = [with_w[0], plain[1], with_w[2]]
    st, seg, rec, pc, w = bd.decompress_device(mixed)
    assert st.cpu().tolist() == [lib.STREAM_OK, lib.STREAM_E_INTENSITY, lib.STREAM_OK], method
    assert not w[1].any() and w[0].cpu().numpy().tobytes() == e2e["want"][0].tobytes() and w[2].cpu().numpy().tobytes() == e2e["want"][2].tobytes()
    with pytest.raises(ValueError, match="frame 1: no valid intensity payload"):
        bd.decompress(mixed)


def test_radius_filter_payload_is_the_compacted_frames(e2e):
    from rpcc_amd.outlier import remove_radius_outlier
    cu, T = e2e["cu"], e2e["T"]
    bc = e2e["pl"].BatchCompressor(T, cluster_num=M, accuracy=ACC, basic_compressor="bzip2", seed=4, intensity_scale=SCALE, radius_outlier_removal=(3, 1.0))
    host = cu.BasicCompressor(method_name="bzip2")
    removed = 0
    # five lone points far out in every frame: the filter has something to remove
    lone = IC.rays(e2e["g"], [3, 5, 7, 9, 11], [100, 400, 700, 1000, 1300], [150.0] * 5, [.5] * 5)
    frames = [np.concatenate([f[:1000], lone, f[1000:]]) for f in e2e["frames"]]
    for b, blob in enumerate(bc.compress(frames)):
        rows = frames[b]
        kept = rows[remove_radius_outlier(rows, nb_points=3, radius=1.0)[1]]
        removed += rows.shape[0] - kept.shape[0]
        want = R.encode_frame(kept, e2e["g"], SCALE)["payload"]
        span = cu.intensity_trailer_span(blob)
        assert bytes(host.decompress(blob[span[0]: span[1]])) == want.tobytes(), b
        assert cu.encode_intensity(T, kept, T.point_cloud_to_range_image(kept), SCALE)[0].tobytes() == want.tobytes()
    assert removed > 0


@pytest.mark.parametrize("kind", ("DBSCAN", "cluster_num=300"))
def test_other_segmentations_carry_it(e2e, kind):
    cu, T = e2e["cu"], e2e["T"]
    kw = dict(segment_method="DBSCAN", max_labels=1023) if kind == "DBSCAN" else dict(cluster_num=300)
    frames = e2e["frames"][:1]
    mk = lambda scale: e2e["pl"].BatchCompressor(T, accuracy=ACC, basic_compressor="bzip2", seed=4, intensity_scale=scale, **kw)
    blob, bare = mk(SCALE).compress(frames)[0], mk(None).compress([frames[0][:, :3]])[0]
    host = cu.BasicCompressor(method_name="bzip2")
    span = cu.intensity_trailer_span(blob)
    assert blob[: len(bare)] == bare and span == (len(bare) + 4, len(blob))
    assert bytes(host.decompress(blob[span[0]: span[1]])) == e2e["refs"][0]["payload"].tobytes()
    out = e2e["dec"](cu.unpack_bitstream(blob, intensity=True), host, T, None if kind == "DBSCAN" else 300, 2 * ACC, None, True, intensity=True)
    assert out[3].tobytes() == e2e["want"][0].tobytes()


def test_streaming_loader_equals_the_batch_compressor(e2e, tmp_path):
    from rpcc_amd.loader import StreamingCompressor
    paths = []
    for i, f in enumerate(e2e["frames"][:2]):
        paths.append(str(tmp_path / ("%d.bin" % i)))
        f.tofile(paths[-1])
    mk = lambda: e2e["pl"].BatchCompressor(e2e["T"], cluster_num=M, accuracy=ACC, basic_compressor="bzip2", seed=4, intensity_scale=SCALE)
    got = {}
    sc = StreamingCompressor(mk(), batch=2, depth=2, workers=2, ingest="rows")
    assert sc.run([(paths, [0, 1])], sink=lambda k, blobs: got.update({k: blobs})) == 2
    assert got[0] == _compress(e2e, "bzip2", {}, True)[:2]
    with pytest.raises(ValueError, match='ingest="rows"'):
        StreamingCompressor(mk(), batch=2, depth=2, workers=2, ingest="xyz")


def test_tools_round_trip(e2e, tmp_path, capsys):
    from rpcc_amd.tools import compress as tc
    from rpcc_amd.tools import decompress as td
    src, out, rec = tmp_path / "frame.bin", tmp_path / "frame.rpcc", tmp_path / "rec.bin"
    e2e["frames"][0].tofile(src)
    base = ["--lidar", GEOM, "--basic_compressor", "bzip2", "--cluster_num", str(M)]
    capsys.readouterr()
    tc.compress(tc.make_parser().parse_args(["--input", str(src), "--output", str(out), "--eval", "--intensity", "--intensity_scale", "100"] + base))
    text = capsys.readouterr().out
    err = float(re.search(r"^    Intensity Error \(max\): +([0-9.eE+-]+)", text, re.M).group(1))
    assert re.search(r"^    Intensity Error \(mean\): ", text, re.M) and err == 0.0            # fl(k / 100) at scale 100: lossless
    td.decompress(td.make_parser().parse_args(["--input", str(out), "--output", str(rec), "--intensity", "--eval", "--original_point_cloud", str(src)] + base))
    assert "Intensity Error (max):  0.0" in capsys.readouterr().out
    got = np.fromfile(rec, np.float32).reshape(-1, 4)
    e = e2e["refs"][0]
    assert got.shape[0] == int((e["ri"] != 0).sum())
    assert np.array_equal(got[:, 3].view(np.uint32), e2e["want"][0].reshape(-1)[e["ri"] != 0].view(np.uint32))
    td.decompress(td.make_parser().parse_args(["--input", str(out), "--output", str(tmp_path / "plain.bin")] + base))
    plain = np.fromfile(tmp_path / "plain.bin", np.float32).reshape(-1, 4)
    assert np.array_equal(plain[:, :3], got[:, :3]) and not plain[:, 3].any()                  # without the flag: today's file
    bare = tmp_path / "bare.rpcc"
    tc.compress(tc.make_parser().parse_args(["--input", str(src), "--output", str(bare)] + base))
    assert open(out, "rb").read()[: os.path.getsize(bare)] == open(bare, "rb").read()
    with pytest.raises(ValueError, match="no intensity trailer"):
        td.decompress(td.make_parser().parse_args(["--input", str(bare), "--output", str(rec), "--intensity"] + base))
