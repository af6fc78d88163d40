"""-m gpu: the hidden_points kernels against tests/hidden_ref.py, bit for bit, on the cases of tests/hidden_cases.py (payload bytes, nbytes,
orphans, uncarried, the decoded points, counts and status with uint8 and uint16 label maps; `crowd` takes a pixel past the 255 cap and a
segment past a workgroup; `past_the_grid` takes the row passes' grid-stride loops through a second trip, tests/hidden_grid_caps.py), each
refusal with its neighbours untouched, the caller-buffer contract, and the channel end to end: the tools on the example rows,
BatchCompressor against the per-frame path with every back-end, with and without intensity and subpixel codes, behind the radius filter,
DBSCAN, NCLT records and the streaming loader."""
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
import hidden_cases as HC  # noqa: E402
import hidden_ref as R  # noqa: E402
import intensity_cases as IC  # noqa: E402
import subpixel_ref as S  # noqa: E402

_CASE, _MEMO = {}, {}


def ref(name, bits):
    """The case's batch with the reference's results per frame: the owner pass once per distinct frame."""
    if name not in _CASE:
        _CASE[name] = HC.CASES[name]()
    batch = _CASE[name]
    return dict(batch, bits=bits, ref=R.encode_frames(batch["frames"], batch["g"], batch["step"], bits, _MEMO.setdefault(name, {})))


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available()
    import __graft_entry__ as ge
    ge.build()
    from rpcc_amd import _lib, compress_utils, ops
    return dict(torch=torch, lib=_lib, ops=ops, cu=compress_utils, dev=torch.device("cuda:0"))


def _upload(env, batch):
    """-> (geom, rows, offsets, ri, max_rows): with batch["pad"] the frames stand between rows that belong to no frame (offsets[0] > 0, rows
    behind offsets[B]); the range images are made of the frames' own rows."""
    torch, ops, g = env["torch"], env["ops"], batch["g"]
    geom = ops.make_geom(g.H, g.W, g.horizontal_FOV, g.vertical_max, g.vertical_min)
    offs = IC.offsets(batch["frames"])
    body = np.concatenate(batch["frames"])
    front, back = batch["pad"] if batch.get("pad") else (np.zeros((0, 4), np.float32),) * 2
    rows = torch.from_numpy(np.concatenate([front, body, back]).astype(np.float32)).to(env["dev"])
    lo = front.shape[0]
    ri = ops.project(rows[lo: lo + body.shape[0]], torch.from_numpy(offs).to(env["dev"]), geom)
    return geom, rows, torch.from_numpy(offs + lo).to(env["dev"]), ri, int(np.diff(offs).max())


def _labels(ri, dtype):
    """A label map whose empty pixels are ri's: 1 where ri == 0, else some other label (0, 2, 3 in turn)."""
    torch = __import__("torch")
    other = (torch.arange(ri.numel(), device=ri.device).view(ri.shape) % 3)
    other = torch.where(other == 1, torch.full_like(other, 3), other)
    lab = torch.where(ri != 0, other, torch.ones_like(other))
    return lab.to(torch.uint8) if dtype == "uint8" else lab.to(torch.int16).view(torch.uint16)


def _tm(env, g):
    return env["torch"].from_numpy(np.ascontiguousarray(IC.orc.transform_map(g), dtype=np.float32)).to(env["dev"])


def _tables(env, g):
    return env["torch"].from_numpy(S.tables(g)).to(env["dev"])


def _check(batch, outs, ri, tag):
    """payload / nbytes / orphans / uncarried of one encode call against the batch's references; -> the host copies of payload and nbytes."""
    g, B = batch["g"], len(batch["frames"])
    P = g.H * g.W
    payload, nbytes, orphans, uncarried = outs
    assert payload.shape[0] == B and orphans.cpu().tolist() == [0] * B, tag
    ph, nh, uh, rh = payload.cpu().numpy(), nbytes.cpu().numpy(), uncarried.cpu().numpy(), ri.cpu().numpy().reshape(B, P)
    bad = []
    for b, e in enumerate(batch["ref"]):
        ok = (np.array_equal(rh[b].view(np.uint32), e["ri"].view(np.uint32)) and nh[b] == e["payload"].shape[0] and uh[b] == e["uncarried"]
              and ph[b, : e["payload"].shape[0]].tobytes() == e["payload"].tobytes())
        if not ok:
            bad.append(b)
    assert not bad, (tag, "frames", bad[:8], [(int(nh[b]), batch["ref"][b]["payload"].shape[0], int(uh[b]), batch["ref"][b]["uncarried"]) for b in bad[:4]])
    return ph, nh


def _decode_all(env, batch, payload, nbytes, ri, tag):
    """The way back with both label widths against the reference, frame by frame."""
    torch, ops, lib, g = env["torch"], env["ops"], env["lib"], batch["g"]
    B, P = len(batch["frames"]), g.H * g.W
    tm, tab = _tm(env, g), _tables(env, g)
    cap = max(e["m"] for e in batch["ref"])
    decs = {}
    for dt in ("uint8", "uint16"):
        out = BA.filled((B, cap, 3), torch.float32, env["dev"], 0xEE)
        pts, cnt, st = ops.hidden_decode(payload, nbytes, _labels(ri, dt), tm, tab, out=out)
        assert st.cpu().tolist() == [lib.STREAM_OK] * B and cnt.cpu().tolist() == [e["m"] for e in batch["ref"]], (tag, dt)
        decs[dt] = pts.cpu().numpy()
    assert decs["uint8"].tobytes() == decs["uint16"].tobytes()
    tmh = tm.cpu().numpy()
    for b, e in enumerate(batch["ref"]):
        want = R.decode_frame(e["payload"], np.where(e["ri"] != 0, 0, 1), g, tmh)
        assert decs["uint8"][b, : e["m"]].view(np.uint32).tobytes() == want.view(np.uint32).tobytes(), (tag, b)
        assert (decs["uint8"][b, e["m"]:].view(np.uint8) == 0xEE).all(), (tag, b, "written past count")


CASES = [("small", b) for b in (0, 1, 4)] + [("round2", b) for b in (0, 1, 4)] + [("crowd", b) for b in (0, 4)] + [("example", 2)]


@pytest.mark.parametrize("name,bits", CASES, ids=["%s-%d" % c for c in CASES])
def test_encode_and_decode_equal_the_reference(env, name, bits):
    ops = env["ops"]
    batch = ref(name, bits)
    geom, rows, offs, ri, max_rows = _upload(env, batch)
    outs = ops.hidden_encode(rows, offs, geom, ri, batch["step"], bits, max_rows=max_rows)
    ph, nh = _check(batch, outs, ri, (name, bits))
    assert outs[0].shape[1] == 16 + batch["g"].H * batch["g"].W + 4 * max_rows
    _decode_all(env, batch, outs[0], outs[1], ri, (name, bits))
    print(name, bits, "n / m / uncarried", [(e["n"], e["m"], e["uncarried"]) for e in batch["ref"]])


def test_the_tool_step_on_the_edge_rows(env):
    """The scenes with the tools' step 0.04, which is no power of two: the division's own rounding decides the codes next to the ties."""
    for name in ("small", "round2"):
        b0 = HC.CASES[name](HC.STEP_TOOL)
        batch = dict(b0, ref=R.encode_frames(b0["frames"], b0["g"], b0["step"], 3))
        geom, rows, offs, ri, max_rows = _upload(env, batch)
        outs = env["ops"].hidden_encode(rows, offs, geom, ri, batch["step"], 3, max_rows=max_rows)
        _check(batch, outs, ri, (name, "step 0.04"))
        _decode_all(env, batch, outs[0], outs[1], ri, (name, "step 0.04"))


def test_a_row_too_short_for_its_frame_is_marked(env):
    """A payload row that holds header and count plane but not the codes: nbytes -1, nothing past the count plane is written, the other
    frames are as ever."""
    torch, ops = env["torch"], env["ops"]
    batch = ref("small", 2)
    g = batch["g"]
    P = g.H * g.W
    geom, rows, offs, ri, max_rows = _upload(env, batch)
    width = max(16 + P, batch["ref"][2]["payload"].shape[0])           # frame 2 fits, frame 0 (more points) does not
    assert batch["ref"][0]["payload"].shape[0] > width
    pay = BA.filled((3, width), torch.uint8, env["dev"], 0xEE)
    _, nb, _, unc = ops.hidden_encode(rows, offs, geom, ri, batch["step"], 2, payload=pay)
    assert nb.cpu().tolist() == [-1, 16, batch["ref"][2]["payload"].shape[0]]
    ph = pay.cpu().numpy()
    n0 = batch["ref"][0]["n"]
    assert ph[0, : 16 + n0].tobytes() == batch["ref"][0]["payload"][: 16 + n0].tobytes() and (ph[0, 16 + n0:] == 0xEE).all()
    assert ph[2, : int(nb[2])].tobytes() == batch["ref"][2]["payload"].tobytes()


def test_past_the_grid_twice_and_from_a_dirty_scratch(env):
    """More rows than one trip of the row passes takes (workgroup 0 takes a second trip) into the caller's buffers: a second call gives the
    same bytes, and so does a call whose scratch holds 0xFF or 0x00 everywhere."""
    import hidden_grid_caps as GC
    torch, ops, dev = env["torch"], env["ops"], env["dev"]
    batch = ref("past_the_grid", 2)
    g, B = batch["g"], len(batch["frames"])
    P = g.H * g.W
    geom, rows, offs, ri, max_rows = _upload(env, batch)
    assert GC.row_trips(rows.shape[0]) == 2
    scratch = torch.empty(env["lib"].lib().rpcc_hidden_scratch_bytes(B, P, rows.shape[0]), dtype=torch.uint8, device=dev)
    outs = dict(payload=torch.empty((B, 16 + P + 4 * max_rows), dtype=torch.uint8, device=dev), nbytes=torch.empty((B,), dtype=torch.int32, device=dev),
                orphans=torch.empty((B,), dtype=torch.int32, device=dev), uncarried=torch.empty((B,), dtype=torch.int32, device=dev))
    first = None
    for tag, fill in (("first", None), ("again", None), ("scratch 0xFF", 0xFF), ("scratch 0x00", 0x00)):
        if fill is not None:
            scratch.fill_(fill)
        for t in outs.values():
            t.zero_()
        got = ops.hidden_encode(rows, offs, geom, ri, batch["step"], 2, scratch=scratch, **outs)
        _check(batch, got, ri, tag)
        if first is None:
            first = got[0].clone()
        assert torch.equal(first, got[0]), tag          # (rows past nbytes included: zeroed before every call and left alone)


def test_the_same_bytes_twice_from_a_dirty_scratch(env):
    """The crowd (thousands of threads race for the slots of one pixel) encoded over and over from scratch contents of every kind: equal bytes."""
    torch, ops, dev = env["torch"], env["ops"], env["dev"]
    batch = ref("crowd", 4)
    g = batch["g"]
    geom, rows, offs, ri, max_rows = _upload(env, batch)
    scratch = torch.empty(env["lib"].lib().rpcc_hidden_scratch_bytes(3, g.H * g.W, rows.shape[0]), dtype=torch.uint8, device=dev)
    seen = set()
    for fill in (0x00, 0xFF, 0x5A, 0x01, 0x80, 0x7F):
        scratch.fill_(fill)
        pay = torch.zeros((3, 16 + g.H * g.W + 4 * max_rows), dtype=torch.uint8, device=dev)
        got = ops.hidden_encode(rows, offs, geom, ri, batch["step"], 4, payload=pay, scratch=scratch)
        _check(batch, got, ri, fill)
        seen.add(got[0].cpu().numpy().tobytes())
    assert len(seen) == 1


def _three(env, bits):
    g, rng = IC.orc.LidarGeom(**HC.SC.SMALL), np.random.default_rng(11)
    batch = dict(g=g, frames=[IC.cloud(g, 90, rng, cols=np.arange(0, g.W, 2)) for _ in range(3)], pad=None)   # (every other column stays empty)
    geom, rows, offs, ri, max_rows = _upload(env, batch)
    payload, nbytes, _, _ = env["ops"].hidden_encode(rows, offs, geom, ri, 0.04, bits, max_rows=max_rows)
    return g, ri, payload, nbytes


@pytest.mark.parametrize("bits", (0, 3))
def test_refusals_write_nothing_of_the_middle_frame(env, bits):
    """Each refusal in the middle frame of three: status E_HIDDEN, count 0 and no point written there, the other two as ever."""
    torch, ops, lib = env["torch"], env["ops"], env["lib"]
    g, ri, payload, nbytes = _three(env, bits)
    P = g.H * g.W
    n1 = int(nbytes[1])
    m = struct.unpack("<I", payload[1, 12:16].cpu().numpy().tobytes())[0]
    n = n1 - 16 - (4 if bits else 2) * m
    assert m >= 8 and 4 <= n < P
    valid = 0x05 if bits else 0x00
    payload[:, 16:][torch.arange(payload.shape[1] - 16, device=payload.device)[None, :] >= (nbytes[:, None] - 16)] = valid     # defined bytes behind every payload
    tm, tab = _tm(env, g), _tables(env, g)
    f32 = lambda v: list(struct.pack("<f", v))
    u32 = lambda v: list(struct.pack("<I", v))

    def damaged(what):
        p, nb, kw = payload.clone(), nbytes.clone(), {}
        put = lambda at, vals: p[1, at: at + len(vals)].copy_(torch.tensor(vals, dtype=torch.uint8))
        if what == "magic":
            put(3, [ord("2")])
        elif what == "subpixel magic":
            put(2, [ord("S")])
        elif what.startswith("bits "):
            put(4, [int(what[5:])])
        elif what.startswith("reserved "):
            put(int(what[9:]), [1])
        elif what.startswith("step "):
            put(8, f32(float(what[5:])))
        elif what == "one more byte":
            nb[1] = n1 + 1
        elif what == "one less byte":
            nb[1] = n1 - 1
        elif what == "m + 1":
            put(12, u32(m + 1))
        elif what == "m + 1 and its bytes":
            put(12, u32(m + 1))
            nb[1] = n1 + (4 if bits else 2)
        elif what == "m - 1 and its bytes":
            put(12, u32(m - 1))
            nb[1] = n1 - (4 if bits else 2)
        elif what == "m huge":
            put(12, u32(0xFFFFFFFF))
        elif what == "a count more":
            put(16, [int(p[1, 16]) + 1])
        elif what == "last count less":
            at = 16 + int(torch.nonzero(p[1, 16: 16 + n]).flatten()[-1])
            put(at, [int(p[1, at]) - 1])
        elif what == "no header":
            nb[1] = 15
        elif what == "no trailer":
            nb[1] = 0
        elif what == "negative":
            nb[1] = -3
        elif what == "past the row":
            nb[1] = p.shape[1] + 2
        elif what == "capacity m - 1":
            kw["capacity"] = m - 1
        elif what == "az code L":
            put(16 + n + 2 * m + 1, [1 << bits])
        elif what == "el code 255":
            put(16 + n + 4 * m - 1, [255])
        elif what == "no tables":
            kw["tables"] = None
        else:
            raise KeyError(what)
        return p, nb, kw

    cases = ["magic", "subpixel magic", "bits 5", "bits 255", "reserved 5", "reserved 6", "reserved 7", "step 0.0", "step -0.04", "step inf", "step nan",
             "one more byte", "one less byte", "m + 1", "m + 1 and its bytes", "m - 1 and its bytes", "m huge", "a count more", "last count less", "no header",
             "no trailer", "negative", "past the row", "capacity m - 1"]
    cases += ["az code L", "el code 255", "no tables", "bits 0"] if bits else ["bits 1"]        # (another width: another length)
    cap = int(max(struct.unpack("<I", payload[b, 12:16].cpu().numpy().tobytes())[0] for b in range(3)))
    for dt in ("uint8", "uint16"):
        lab = _labels(ri, dt)
        good, gc, st = ops.hidden_decode(payload, nbytes, lab, tm, tab, out=BA.filled((3, cap, 3), torch.float32, env["dev"], 0xEE))
        assert st.cpu().tolist() == [0, 0, 0] and int(gc[1]) == m
        for what in cases:
            p, nb, kw = damaged(what)
            c = kw.pop("capacity", cap)
            tables = kw.pop("tables", tab)
            out = BA.filled((3, c, 3), torch.float32, env["dev"], 0xEE)
            pts, cnt, st = ops.hidden_decode(p, nb, lab, tm, tables, out=out)
            if what == "capacity m - 1" or (what == "no tables"):
                others_ok = [int(v) <= c for v in gc.cpu().tolist()] if what == "capacity m - 1" else [False, False, False]
                assert int(st[1]) == lib.STREAM_E_HIDDEN and int(cnt[1]) == 0 and (pts[1].view(torch.uint8) == 0xEE).all(), (dt, what)
                for b in (0, 2):
                    assert (int(st[b]) == lib.STREAM_OK) == others_ok[b], (dt, what, b)
                continue
            assert st.cpu().tolist() == [lib.STREAM_OK, lib.STREAM_E_HIDDEN, lib.STREAM_OK], (dt, what)
            assert cnt.cpu().tolist() == [int(gc[0]), 0, int(gc[2])] and (pts[1].view(torch.uint8) == 0xEE).all(), (dt, what)
            assert torch.equal(pts[0], good[0]) and torch.equal(pts[2], good[2]), (dt, what)
    # a label map with another number of non-empty pixels refuses too
    lab = _labels(ri, "uint8").clone()
    empty = torch.nonzero(lab[1].reshape(-1) == 1).flatten()
    lab[1].view(-1)[empty[0]] = 0
    out = BA.filled((3, cap, 3), torch.float32, env["dev"], 0xEE)
    pts, cnt, st = ops.hidden_decode(payload, nbytes, lab, tm, tab, out=out)
    assert st.cpu().tolist() == [0, lib.STREAM_E_HIDDEN, 0] and (pts[1].view(torch.uint8) == 0xEE).all()


@pytest.mark.parametrize("pattern", ("ones", "intmax", "nan", "alt(0,0)", "alt(0,1)", "half(0)", "half(1)"))
def test_buffer_contract(env, pattern):
    """Exact-size buffers between guard bytes, the scratch filled with a hostile pattern: nothing outside nbytes bytes of a payload row or
    outside any buffer is written, every other output byte is, the results do not depend on what the scratch held, and the decoder reads
    nothing past nbytes and writes nothing past count."""
    torch, ops, dev = env["torch"], env["ops"], env["dev"]
    bits = 4
    for name in ("small", "crowd"):
        batch = ref(name, bits)
        g, B = batch["g"], len(batch["frames"])
        P = g.H * g.W
        geom, rows, offs, ri, max_rows = _upload(env, batch)
        width = 16 + P + 4 * max_rows
        need = env["lib"].lib().rpcc_hidden_scratch_bytes(B, P, rows.shape[0])
        arenas = dict(scratch=BA.Arena(need, dev, back=1 << 16), payload=BA.Arena(B * width, dev, back=1 << 16), nbytes=BA.Arena(4 * B, dev, back=4096),
                      orphans=BA.Arena(4 * B, dev, back=4096), uncarried=BA.Arena(4 * B, dev, back=4096))

        def run(fill):
            for k, a in arenas.items():
                a.fill(pattern if k == "scratch" else "zero")
                if k != "scratch":
                    a.view.fill_(fill)
            ops.hidden_encode(rows, offs, geom, ri, batch["step"], bits, payload=arenas["payload"].view.view(B, width),
                              nbytes=arenas["nbytes"].view.view(torch.int32), orphans=arenas["orphans"].view.view(torch.int32),
                              uncarried=arenas["uncarried"].view.view(torch.int32), scratch=arenas["scratch"].view)
            torch.cuda.synchronize()
            for k, a in arenas.items():
                assert a.check_guards() is None, (name, pattern, k, a.check_guards())
            return {k: a.view.clone() for k, a in arenas.items() if k != "scratch"}

        outs = {}
        holes = BA.unwritten(run, outs)
        nb = outs["nbytes"].view(torch.int32).cpu().numpy()
        want_holes = (np.arange(width)[None, :] >= nb[:, None]).reshape(-1)
        assert np.array_equal(holes["payload"].cpu().numpy(), want_holes), (name, pattern)
        for k in ("nbytes", "orphans", "uncarried"):
            assert not holes[k].any(), (name, pattern, k)
        assert not outs["orphans"].view(torch.int32).any()
        assert outs["uncarried"].view(torch.int32).cpu().tolist() == [e["uncarried"] for e in batch["ref"]]
        for b, e in enumerate(batch["ref"]):
            assert outs["payload"].view(B, width)[b, : nb[b]].cpu().numpy().tobytes() == e["payload"].tobytes(), (name, pattern, b)
        # the way back: exact-size inputs and output, and nothing past nbytes is read (two fillings of the rows' tails, one result)
        lab, tm, tab = _labels(ri, "uint8"), _tm(env, g), _tables(env, g)
        cap = max(e["m"] for e in batch["ref"])
        res = []
        for fill in (0x00, 0xFF):
            pay = BA.Arena(B * width, dev, back=1 << 16)
            pay.view.copy_(outs["payload"])
            pv = pay.view.view(B, width)
            pv[torch.from_numpy(want_holes.reshape(B, width)).to(dev)] = fill
            out, cnt, st = BA.Arena(12 * B * cap, dev, back=1 << 16), BA.Arena(4 * B, dev, back=4096), BA.Arena(4 * B, dev, back=4096)
            out.view.fill_(0xEE)
            ops.hidden_decode(pv, outs["nbytes"].view(torch.int32), lab, tm, tab, out=out.view.view(torch.float32).view(B, cap, 3),
                              count=cnt.view.view(torch.int32), status=st.view.view(torch.int32))
            torch.cuda.synchronize()
            assert out.check_guards() is None and st.check_guards() is None and cnt.check_guards() is None and pay.check_guards() is None
            assert not st.view.any() and cnt.view.view(torch.int32).cpu().tolist() == [e["m"] for e in batch["ref"]]
            res.append(out.view.clone())
        assert torch.equal(res[0], res[1])
        tmh = tm.cpu().numpy()
        for b, e in enumerate(batch["ref"]):
            got = res[0].view(torch.float32).view(B, cap, 3)[b].cpu().numpy()
            assert got[: e["m"]].view(np.uint32).tobytes() == R.decode_frame(e["payload"], np.where(e["ri"] != 0, 0, 1), g, tmh).view(np.uint32).tobytes()
            assert (got[e["m"]:].view(np.uint8) == 0xEE).all()


def test_orphans_are_counted(env):
    """A range image that is not the image of the rows: the pixels no row owns are counted per frame; every row of such a pixel is hidden."""
    torch, ops = env["torch"], env["ops"]
    batch = ref("small", 0)
    geom, rows, offs, ri, max_rows = _upload(env, batch)
    ri2 = ri.clone()
    empty = torch.nonzero(ri2[2].reshape(-1) == 0).flatten()
    ri2[2].view(-1)[empty[:3]] = 5.0                       # three pixels nobody owns
    _, nbytes, orphans, _ = ops.hidden_encode(rows, offs, geom, ri2, batch["step"], 0, max_rows=max_rows)
    assert orphans.cpu().tolist() == [0, 0, 3] and int(nbytes[2]) >= batch["ref"][2]["payload"].shape[0] + 3


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
ACC, GEOM, M, SCALE, BITS = 0.02, "VelodyneVLP16", 40, 100.0, 2
# every back-end of compress_utils.BACKENDS, host and device coders alike (tests/test_gpu_intensity.py: the same list)
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
        extra = xyz[rng.integers(0, xyz.shape[0], 3000 + 500 * i), :3] * rng.uniform(1.0, 1.6, (3000 + 500 * i, 1)).astype(np.float32)   # points behind others, on their rays
        xyz = np.concatenate([xyz[:, :3], extra])[rng.permutation(xyz.shape[0] + extra.shape[0])]
        frames.append(np.ascontiguousarray(np.concatenate([xyz, (rng.integers(0, 100, xyz.shape[0]) / np.float32(100))[:, None]], 1), dtype=np.float32))
    T = dataset.build_dataset(lidar_type=GEOM).PCTransformer
    memo = {}
    refs = {bits: R.encode_frames(frames, g, 2 * ACC, bits, memo) for bits in (0, BITS)}
    assert all(e["m"] > 1000 for e in refs[0])
    return dict(env, pl=pipeline, dec=decode_frame, T=T, g=g, frames=frames, refs=refs, cache={})


def _compress(e2e, method, kw, intensity, subpixel, hidden, xyz_only=False):
    key = (method, tuple(sorted(kw.items())), intensity, subpixel, hidden, xyz_only)
    if key not in e2e["cache"]:
        bc = e2e["pl"].BatchCompressor(e2e["T"], cluster_num=M, accuracy=ACC, basic_compressor=method, seed=4, intensity_scale=SCALE if intensity else None,
                                       subpixel_bits=BITS if subpixel else None, hidden_points=hidden, **kw)
        e2e["cache"][key] = bc.compress([f[:, :3] for f in e2e["frames"]] if xyz_only else e2e["frames"])
        if hidden:
            assert bc.hidden_uncarried.tolist() == [e["uncarried"] for e in e2e["refs"][0]]
            assert bc.hidden_carried.tolist() == [e["m"] for e in e2e["refs"][0]]
    return e2e["cache"][key]


@pytest.mark.parametrize("intensity,subpixel", ((False, False), (True, False), (False, True), (True, True)), ids=("plain", "intensity", "subpixel", "both"))
@pytest.mark.parametrize("method,kw", BACKENDS, ids=[m + "".join("+" + k for k in kw) for m, kw in BACKENDS])
def test_batch_compressor_equals_the_per_frame_path(e2e, method, kw, intensity, subpixel):
    cu, T, g = e2e["cu"], e2e["T"], e2e["g"]
    bits = BITS if subpixel else 0
    refs = e2e["refs"][bits]
    assert {m for m, _ in BACKENDS} == set(cu.BACKENDS)
    with_h, bare = _compress(e2e, method, kw, intensity, subpixel, True), _compress(e2e, method, kw, intensity, subpixel, False)

    def same(x, y, tag):
        """Two containers byte for byte; where separate gzip.compress calls on the host wrote them, but for the members' MTIME bytes."""
        if method in ("gzip", "deflate") and not kw:
            GZ.assert_equal_but_mtime(x, y, tag)
        else:
            assert x == y, tag

    if not intensity:
        for b, (x, y) in enumerate(zip(_compress(e2e, method, kw, False, subpixel, True, xyz_only=True), with_h)):
            same(x, y, (method, b, "[N,3] frames"))                                              # a zero fourth column on the host
    bc = cu.BasicCompressor(method_name=method, **kw)
    host = cu.BasicCompressor(method_name=method)
    tmh = T.transform_map.reshape(-1, 3)
    for b, (blob, base) in enumerate(zip(with_h, bare)):
        same(blob[: len(base)], base, (method, b, "prefix"))                                     # the bytes before the trailer: the container without it
        assert len(blob) > len(base) + 4, (method, b)
        cd = cu.unpack_bitstream(blob, intensity=intensity, subpixel=subpixel, hidden_points=True)
        assert tuple(cd)[-1] == "hidden_points" and len(base) + 4 + len(cd["hidden_points"]) == len(blob)
        assert bytes(host.decompress(cd["hidden_points"])) == refs[b]["payload"].tobytes(), (method, b)
        # the per-frame path: the frame's rows against its own range image, through compress_point_cloud's arguments
        plain = cu.unpack_bitstream(base)
        nrows = len(host.decompress(plain["plane_param"])) // 16
        rq, idx_map, sal, plane = cu.decompress_point_cloud(plain, host, nrows, T.H, T.W)
        ri = T.point_cloud_to_range_image(e2e["frames"][b])
        hpay, uncarried = cu.encode_hidden(T, e2e["frames"][b][:, :3] if b == 1 else e2e["frames"][b], ri, 2 * ACC, bits)
        assert hpay.tobytes() == refs[b]["payload"].tobytes() and uncarried == refs[b]["uncarried"]
        ipay = cu.encode_intensity(T, e2e["frames"][b], ri, SCALE)[0] if intensity else None
        spay = cu.encode_subpixel(T, e2e["frames"][b], ri, BITS)[0] if subpixel else None
        original, compressed = cu.compress_point_cloud(bc, plane, idx_map, sal, rq, intensity=ipay, subpixel=spay, hidden_points=hpay)
        assert ("intensity" in original) == intensity and ("subpixel" in original) == subpixel and original["hidden_points"].tobytes() == hpay.tobytes()
        same(blob, cu.pack_bitstream(compressed), (method, b, "per frame"))
        # the way back: the image points, then the reference's hidden points
        rec, pc, seg, *w = e2e["dec"](cd, host, T, M, 2 * ACC, None, True, intensity=intensity, subpixel=subpixel, hidden_points=True)
        rec0, pc0, seg0, *w0 = e2e["dec"](cu.unpack_bitstream(base, intensity=intensity, subpixel=subpixel), host, T, M, 2 * ACC, None, True,
                                          intensity=intensity, subpixel=subpixel)                 # the container without the trailer: today's result
        # a reader that asks for nothing reads the geometry as ever (separate gzip.compress calls: but for the members' MTIME bytes)
        plain = [{k: v[:4] + v[8:] if isinstance(v, bytes) and v[:3] == b"\x1f\x8b\x08" else v for k, v in cu.unpack_bitstream(c).items()} for c in (blob, base)]
        assert plain[0] == plain[1]
        if intensity or subpixel:                                                                 # one that asks for the older trailers only is told what is missing
            with pytest.raises(ValueError, match="hidden_points=True"):
                cu.unpack_bitstream(blob, intensity=intensity, subpixel=subpixel)
        want = R.decode_frame(refs[b]["payload"], seg.reshape(-1), g, tmh)
        P = T.H * T.W
        assert pc.dtype == np.float32 and pc.shape == (P + refs[b]["m"], 3)
        assert pc[:P].tobytes() == pc0.reshape(-1, 3).tobytes() and pc[P:].view(np.uint32).tobytes() == want.view(np.uint32).tobytes(), (method, b)
        assert rec0.tobytes() == rec.tobytes() and seg0.tobytes() == seg.tobytes() and len(w) == (1 if intensity else 0)
        if intensity:
            assert w[0].tobytes() == w0[0].tobytes() and w[0].shape == (T.H, T.W)
        with pytest.raises(ValueError, match="no hidden_points trailer"):
            cu.unpack_bitstream(base, intensity=intensity, subpixel=subpixel, hidden_points=True)
    # a damaged payload: decode_frame refuses by name
    cd = cu.unpack_bitstream(with_h[0], intensity=intensity, subpixel=subpixel, hidden_points=True)
    raw = bytearray(host.decompress(cd["hidden_points"]))
    raw[16] += 1
    with pytest.raises(ValueError, match="hidden_points payload: the counts sum to"):
        e2e["dec"](dict(cd, hidden_points=host.compress(np.frombuffer(bytes(raw), np.uint8))), host, T, M, 2 * ACC, None, True, intensity=intensity,
                   subpixel=subpixel, hidden_points=True)


def test_radius_filter_and_dbscan(e2e):
    from rpcc_amd.outlier import remove_radius_outlier
    cu, T, g = e2e["cu"], e2e["T"], e2e["g"]
    host = cu.BasicCompressor(method_name="bzip2")
    bc = e2e["pl"].BatchCompressor(T, cluster_num=M, accuracy=ACC, basic_compressor="bzip2", seed=4, hidden_points=True, radius_outlier_removal=(3, 1.0))
    lone = IC.rays(g, [3, 5, 7, 9, 11], [100, 400, 700, 1000, 1300], [150.0] * 5, [.5] * 5)     # five lone points far out: the filter has something to remove
    frames = [np.concatenate([f[:1000], lone, f[1000:]]) for f in e2e["frames"][:2]]
    removed = 0
    for b, blob in enumerate(bc.compress(frames)):
        kept = frames[b][remove_radius_outlier(frames[b], nb_points=3, radius=1.0)[1]]
        removed += frames[b].shape[0] - kept.shape[0]
        want = R.encode_frame(kept, g, 2 * ACC, 0)["payload"]
        assert bytes(host.decompress(cu.unpack_bitstream(blob, hidden_points=True)["hidden_points"])) == want.tobytes(), b
    assert removed > 0
    mk = lambda on: e2e["pl"].BatchCompressor(T, accuracy=ACC, basic_compressor="bzip2", seed=4, subpixel_bits=BITS, intensity_scale=SCALE,
                                              segment_method="DBSCAN", max_labels=1023, hidden_points=on)
    blob, base = mk(True).compress(e2e["frames"][:1])[0], mk(False).compress(e2e["frames"][:1])[0]
    cd = cu.unpack_bitstream(blob, intensity=True, subpixel=True, hidden_points=True)
    assert blob[: len(base)] == base and bytes(host.decompress(cd["hidden_points"])) == e2e["refs"][BITS][0]["payload"].tobytes()
    rec, pc, seg, w = e2e["dec"](cd, host, T, None, 2 * ACC, None, True, intensity=True, subpixel=True, hidden_points=True)
    want = R.decode_frame(e2e["refs"][BITS][0]["payload"], seg.reshape(-1), g, T.transform_map.reshape(-1, 3))
    assert pc[T.H * T.W:].view(np.uint32).tobytes() == want.view(np.uint32).tobytes()


def test_nclt_records_and_streaming_loader(e2e, tmp_path):
    from rpcc_amd import records
    from rpcc_amd.loader import StreamingCompressor
    cu, T, g = e2e["cu"], e2e["T"], e2e["g"]
    host = cu.BasicCompressor(method_name="bzip2")
    paths = []
    for i, f in enumerate(e2e["frames"]):
        paths.append(str(tmp_path / ("%d.bin" % i)))
        f.tofile(paths[-1])
    mk = lambda **kw: e2e["pl"].BatchCompressor(T, cluster_num=M, accuracy=ACC, basic_compressor="bzip2", seed=4, hidden_points=True, **kw)
    got = {}
    bc = mk(intensity_scale=SCALE, subpixel_bits=BITS)
    sc = StreamingCompressor(bc, batch=2, depth=2, workers=2, ingest="rows")
    # two batches through the slots: the second one's frame is the largest (its payload rows are longer than the first batch's)
    assert sc.run([(paths[:2], [0, 1]), (paths[2:], [2])], sink=lambda k, blobs: got.update({k: blobs})) == 3
    assert got[0] + got[1] == _compress(e2e, "bzip2", {}, True, True, True)
    assert bc.hidden_totals == [sum(e["m"] for e in e2e["refs"][BITS]), sum(e["uncarried"] for e in e2e["refs"][BITS])]
    with pytest.raises(ValueError, match='ingest="rows"'):
        StreamingCompressor(mk(), batch=2, depth=2, workers=2, ingest="xyz")
    # NCLT records: the rows the device unpacks are the rows of records.unpack_host
    rng = np.random.default_rng(5)
    rec = np.zeros((4000, records.RECORD_BYTES), np.uint8)
    rec[:, :6] = rng.integers(0, 256, (4000, 6))
    rec[:, 1:6:2] = rng.integers(70, 86, (4000, 3))                # the high bytes: coordinates within ten metres
    rec[:, 6] = rng.integers(0, 256, 4000)
    blob = mk(point_format="nclt").compress([rec])[0]
    e = R.encode_frame(records.unpack_host(rec), g, 2 * ACC, 0)
    assert e["m"] > 0 and bytes(host.decompress(cu.unpack_bitstream(blob, hidden_points=True)["hidden_points"])) == e["payload"].tobytes()


def test_tools_round_trip_on_the_example_rows(env, tmp_path, capsys):
    """tools/compress.py then tools/decompress.py with --hidden_points at --accuracy 0.02 on the example rows: the points written are the
    image points and the reference's hidden points, 122 320 together, nothing uncarried, and nearer to the original than the image alone."""
    from rpcc_amd import evaluate_metrics as em
    from rpcc_amd.tools import compress as tc
    from rpcc_amd.tools import decompress as td
    cu = env["cu"]
    batch = ref("example", 0)
    g, rows, e = batch["g"], batch["frames"][0], batch["ref"][0]
    golden = np.load(os.path.join(HC.SC.GOLDEN, "example_64E.npz"))
    src, out, rec_f, bare_f = tmp_path / "frame.bin", tmp_path / "frame.rpcc", tmp_path / "rec.bin", tmp_path / "bare.bin"
    rows.tofile(src)
    base = ["--lidar", "Velodyne64E", "--basic_compressor", "bzip2", "--accuracy", "0.02"]
    capsys.readouterr()
    tc.compress(tc.make_parser().parse_args(["--input", str(src), "--output", str(out), "--eval", "--hidden_points"] + base))
    text = capsys.readouterr().out
    assert "(hidden_points: the image points and the hidden points against the original points)" in text
    assert re.search(r"Hidden points carried: +%d\b" % e["m"], text) and "not carried" not in text
    td.decompress(td.make_parser().parse_args(["--input", str(out), "--output", str(rec_f), "--hidden_points"] + base))
    assert re.search(r"Hidden points: +%d\b" % e["m"], capsys.readouterr().out)
    td.decompress(td.make_parser().parse_args(["--input", str(out), "--output", str(bare_f)] + base))       # a reader that does not ask
    got, bare = np.fromfile(rec_f, np.float32).reshape(-1, 4), np.fromfile(bare_f, np.float32).reshape(-1, 4)
    assert e["uncarried"] == 0 and e["n"] + e["m"] == rows.shape[0] == 122320 and e["n"] == 94053
    nb = bare.shape[0]                                     # (the save rule drops a point whose coordinates sum to 0)
    assert nb <= e["n"] and got[:nb].tobytes() == bare.tobytes()
    host = cu.BasicCompressor(method_name="bzip2")
    cd = cu.read_compressed_bitstream(str(out), hidden_points=True)
    assert bytes(host.decompress(cd["hidden_points"])) == e["payload"].tobytes()
    # the reference applied to the golden range image: its non-empty pixels are the golden label map's
    labels = golden["seg_idx"].reshape(-1)
    assert np.array_equal(labels != 1, e["ri"] != 0)
    T = __import__("rpcc_amd.dataset", fromlist=["x"]).build_dataset(lidar_type="Velodyne64E").PCTransformer
    want = R.decode_frame(e["payload"], labels, g, T.transform_map.reshape(-1, 3))
    saved = lambda pts: pts[np.sum(pts, -1) != 0]
    assert got[nb:, :3].view(np.uint32).tobytes() == saved(want).view(np.uint32).tobytes() and not got[nb:, 3].view(np.uint32).any()
    assert saved(want).shape[0] == e["m"] and nb == e["n"] and got.shape[0] == 122320      # nothing of this sweep is dropped by the rule
    with_h = em.calc_chamfer_distance(rows[:, :3], got[:, :3], out=False)["mean"]
    without = em.calc_chamfer_distance(rows[:, :3], bare[:, :3], out=False)["mean"]
    print("Chamfer (mean) with / without the trailer:", with_h, without)
    assert with_h < without
    # with --subpixel 2 the trailer carries lateral codes, with --intensity the hidden rows' fourth column is +0.0
    e2 = ref("example", 2)["ref"][0]
    tc.compress(tc.make_parser().parse_args(["--input", str(src), "--output", str(out), "--hidden_points", "--subpixel", "2", "--intensity"] + base))
    cd = cu.read_compressed_bitstream(str(out), intensity=True, subpixel=True, hidden_points=True)
    assert bytes(host.decompress(cd["hidden_points"])) == e2["payload"].tobytes()
    td.decompress(td.make_parser().parse_args(["--input", str(out), "--output", str(rec_f), "--hidden_points", "--subpixel", "--intensity"] + base))
    got2 = np.fromfile(rec_f, np.float32).reshape(-1, 4)
    want2 = R.decode_frame(e2["payload"], np.where(e2["ri"] != 0, 0, 1), g, T.transform_map.reshape(-1, 3))
    nb2 = got2.shape[0] - saved(want2).shape[0]
    assert got2[nb2:, :3].view(np.uint32).tobytes() == saved(want2).view(np.uint32).tobytes() and got2.shape[0] == 122320
    assert not got2[nb2:, 3].view(np.uint32).any()          # +0.0: the trailer carries no intensity
