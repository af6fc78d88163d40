"""librpcc_fields.so on the GPU: pointfile.unpack bit-equal to the host reader on the whole table of tests/pointfile_cases.py in one call, at
the point counts where a tile ends (tests/fields_caps.py) for every stride the kernel stages differently, on frames that abut byte to byte,
past the capped grid's first trip in both grid dimensions, inside guard bytes with hostile prior contents, and on refused descriptors."""
import numpy as np
import pytest
import torch

import buffer_arena as BA
import fields_caps as FC
import fields_ref as FR
import pointfile_cases as PC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as ge
    ge.build()
    from rpcc_amd import pointfile
    assert torch.cuda.is_available()
    return dict(pf=pointfile, dev=torch.device("cuda:0"))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def run(env, chunk, desc, tail=0):
    """chunk uint8 (numpy), desc int64 [B,16] -> (rows, row_offsets, status) as numpy.  tail: bytes of the device allocation behind the chunk
    (the chunk tensor is a view of its first bytes), so that a read past nbytes would still be inside the test's allocation."""
    buf = torch.full((chunk.size + tail,), 0x5A, dtype=torch.uint8, device=env["dev"])
    buf[:chunk.size] = torch.from_numpy(np.array(chunk, dtype=np.uint8)).to(env["dev"])
    rows, offs, status = env["pf"].unpack(buf[:chunk.size], desc)
    torch.cuda.synchronize()
    assert rows.dtype == torch.float32 and rows.dim() == 2 and rows.shape[1] == 4 and status.dtype == torch.int32
    return rows.cpu().numpy(), offs.cpu().numpy(), status.cpu().numpy()


def run_into(env, chunk, desc, offs, tail=0):
    """The same through pointfile.unpack_into, with the test's own row_offsets (pointfile.unpack makes them of the descriptors' counts)."""
    dev = env["dev"]
    buf = torch.full((chunk.size + tail,), 0x5A, dtype=torch.uint8, device=dev)
    buf[:chunk.size] = torch.from_numpy(np.array(chunk, dtype=np.uint8)).to(dev)
    total = int(offs[-1])
    rows = torch.full((total, 4), float("nan"), dtype=torch.float32, device=dev)
    status = torch.full((desc.shape[0],), -7, dtype=torch.int32, device=dev)
    env["pf"].unpack_into(buf[:chunk.size], torch.from_numpy(desc).to(dev), torch.from_numpy(offs).to(dev), total, rows, status)
    torch.cuda.synchronize()
    return rows.cpu().numpy(), status.cpu().numpy()


def test_the_whole_table_in_one_call(env):
    """Mixed layouts, one descriptor per frame: records of every step of the table behind their headers, planes, stored rows."""
    pf = env["pf"]
    frames = [FR.case_frame(pf, c) for c in PC.ACCEPTED]
    host = np.concatenate([pf.read_rows(c[2], name=c[0], fmt=c[1]) for c in PC.ACCEPTED])
    for kw in (dict(), dict(lead=5)):
        chunk, desc, offs, want = FR.build_chunk(frames, **kw)
        rows, got_offs, status = run(env, chunk, desc)
        assert np.array_equal(got_offs, offs) and not status.any()
        assert np.array_equal(bits(rows), bits(host)) and np.array_equal(bits(rows), bits(want)), kw


LAYOUTS = {"step12": dict(step=12, types=(FR.F32, FR.F32, FR.F32, FR.NONE)), "step16": dict(step=16), "step22": dict(step=22), "step32": dict(step=32),
           "step256": dict(step=256, types=(FR.F64, FR.F32, FR.I16, FR.U8)), "planes": dict(step=0, plane=True, types=(FR.F32, FR.F64, FR.F32, FR.U16))}


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_point_counts_around_a_tile(env, name):
    """Every count as a frame of one call, each frame at an odd span_off."""
    kw = LAYOUTS[name]
    max_step = 8 if kw.get("plane") else kw["step"]
    counts = FC.point_counts(max_step)
    t = FC.tile_rows(max_step)
    assert counts[2:5] == (t - 1, t, t + 1) and counts[5] > 3 * t and (counts[5] % t) % 64 != 0
    assert (t == FC.TILE_MAX_ROWS) == (max_step * FC.TILE_MAX_ROWS <= FC.STAGE_BYTES)
    rng = np.random.default_rng(11)
    if kw.get("plane"):      # and a frame whose four planes lie further apart than one stage holds: the columns are staged one after the other
        counts += (5 * t + 37,)
        assert counts[-1] * 4 > FC.STAGE_BYTES + 16
    frames = [FR.record_frame(rng, n, **kw) for n in counts]
    if kw.get("plane"):      # and one without an intensity plane: its fourth column is written as +0.0
        frames.append(FR.record_frame(rng, counts[-1], 0, plane=True, types=(FR.F32, FR.F32, FR.I32, FR.NONE)))
    chunk, desc, offs, want = FR.build_chunk(frames, lead=1 if name != "step16" else 0)
    assert name == "step16" or all(d[0] % 2 == 1 for d in desc)
    rows, _, status = run(env, chunk, desc)
    assert not status.any() and np.array_equal(bits(rows), bits(want))


def test_frames_that_abut(env):
    """Frames byte to byte behind one another, the last one ending with the chunk at an address that is no multiple of 16: a stage that
    over-reads takes the next frame's bytes for its own, or reads past the chunk."""
    rng = np.random.default_rng(12)
    frames = [FR.record_frame(rng, n, step, types=ty) for n, step, ty in ((300, 22, (FR.F32,) * 4), (1, 13, (FR.F32, FR.F32, FR.F32, FR.U8)), (257, 12, (FR.F32, FR.F32, FR.F32, FR.NONE)),
                                                                           (64, 29, (FR.F64, FR.F64, FR.F64, FR.I8)), (513, 22, (FR.F32,) * 4))]
    frames.append(FR.record_frame(rng, 259, 0, plane=True, types=(FR.F32, FR.F32, FR.F32, FR.F32)))
    chunk, desc, offs, want = FR.build_chunk(frames, abut=True)
    assert chunk.size % 16 and [int(d[0]) for d in desc[1:]] == np.cumsum([len(f[0]) for f in frames])[:-1].tolist()
    rows, _, status = run(env, chunk, desc)
    assert not status.any() and np.array_equal(bits(rows), bits(want))
    # and with the device allocation ending where the chunk ends, up to the allocator's rounding
    rows, _, status = run(env, chunk[: desc[-1][0]], desc[:-1])
    assert not status.any() and np.array_equal(bits(rows), bits(want[: offs[-2]]))


def test_past_the_capped_grid_in_both_dimensions(env):
    rng = np.random.default_rng(13)
    ty = (FR.F32, FR.F32, FR.F32, FR.NONE)
    # tiles: one frame of more tiles than the capped grid has workgroups -- a full first trip and a partial second one that ends inside a wavefront
    t = FC.tile_rows(12)
    n = t * (FC.FLD_GRID_CAP + 5) + 37
    assert FC.grid(n, 1) == (FC.FLD_GRID_CAP, 1) and FC.FLD_GRID_CAP < -(-n // t) < 2 * FC.FLD_GRID_CAP and (n % t) % 64 and 28 * n < 64 << 20
    chunk, desc, offs, want = FR.build_chunk([FR.record_frame(rng, n, 12, types=ty)], lead=3)
    rows, _, status = run(env, chunk, desc)
    assert not status.any() and np.array_equal(bits(rows), bits(want))
    # and one frame far larger than the average frame the grid was sized for, among many: several trips over its tiles
    B = 64
    small = [FR.record_frame(rng, 300, 12, types=ty) for _ in range(B - 1)]
    big_n = t * 37 + 37
    frames = small[:10] + [FR.record_frame(rng, big_n, 12, types=ty)] + small[10:]
    chunk, desc, offs, want = FR.build_chunk(frames, lead=3)
    fx, fy = FC.grid(int(offs[-1]), B)
    assert fy == B and fx * fy <= FC.FLD_GRID_CAP and -(-big_n // t) > 3 * fx
    rows, _, status = run(env, chunk, desc)
    assert not status.any() and np.array_equal(bits(rows), bits(want))
    # frames: more frames than the grid has rows
    B = FC.FLD_GRID_CAP + 70
    frames = [FR.record_frame(rng, int(n), 22) for n in rng.integers(0, 6, B)]
    frames[-1] = FR.record_frame(rng, 300, 22)
    chunk, desc, offs, want = FR.build_chunk(frames, abut=True)
    assert FC.grid(int(offs[-1]), B) == (1, FC.FLD_GRID_CAP)
    rows, _, status = run(env, chunk, desc)
    assert status.shape == (B,) and not status.any() and np.array_equal(bits(rows), bits(want))


@pytest.mark.parametrize("pattern", ("nan", "ones", "half(1)"))
def test_outputs_between_guards_over_hostile_contents(env, pattern):
    """rows of exactly total * 16 bytes and status of exactly B * 4 between guard bytes, pre-filled: every row and every status word is written,
    nothing else is, and a second run over other contents gives the same bits."""
    from rpcc_amd._fields_lib import check, lib
    from rpcc_amd._lib import ptr, stream
    dev = env["dev"]
    rng = np.random.default_rng(14)
    frames = [FR.record_frame(rng, n, step, types=ty) for n, step, ty in ((1000, 22, (FR.F32,) * 4), (0, 16, (FR.F32,) * 4), (1, 12, (FR.F32, FR.F32, FR.F32, FR.NONE)),
                                                                           (77, 256, (FR.F32, FR.F32, FR.F32, FR.U32)))]
    bad = FR.record_frame(rng, 40, 22)
    bad[1][7] = 2                                   # a step below the size: its rows must be written too, as +0.0
    frames.insert(2, (bad[0], bad[1], np.zeros((40, 4), np.float32)))
    chunk, desc, offs, want = FR.build_chunk(frames, lead=7)
    B, total = desc.shape[0], int(offs[-1])
    src = torch.from_numpy(chunk).to(dev)
    desc_d, offs_d = torch.from_numpy(desc).to(dev), torch.from_numpy(offs).to(dev)
    a_rows = BA.Arena(16 * total, device=dev, front=4096, back=1 << 16).fill(pattern)
    a_stat = BA.Arena(4 * B, device=dev, front=4096, back=4096).fill(pattern)
    rows, status = a_rows.view.view(torch.float32).view(total, 4), a_stat.view.view(torch.int32)
    check(lib().rpcc_fields_unpack(ptr(src), src.numel(), ptr(desc_d), B, ptr(offs_d), total, ptr(rows), ptr(status), stream()))
    torch.cuda.synchronize()
    assert a_rows.check_guards() is None and a_stat.check_guards() is None
    assert status.cpu().tolist() == [0, 0, FR.E_LAYOUT, 0, 0]
    assert np.array_equal(bits(rows.cpu().numpy()), bits(want))


def test_refused_descriptors(env):
    """A range past the span, a step below the size, a row count that disagrees, and the others of tests/test_fields_core_host.py, between good
    frames: E_LAYOUT, +0.0 rows, the neighbours' rows untouched.  Every byte a refused descriptor names still lies inside the chunk."""
    rng = np.random.default_rng(15)
    goods = [FR.record_frame(rng, 300, 22), FR.record_frame(rng, 50, 12, types=(FR.F32, FR.F32, FR.F32, FR.NONE)), FR.record_frame(rng, 513, 32)]
    bad = []
    for edit in (lambda d: d.__setitem__(3 + 2, d[3 + 2] + 12), lambda d: d.__setitem__(7 + 0, 3), lambda d: d.__setitem__(2, 49),
                 lambda d: d.__setitem__(7 + 1, 257), lambda d: d.__setitem__(11 + 1, 0), lambda d: d.__setitem__(11 + 3, 9),
                 lambda d: d.__setitem__(3 + 1, -1), lambda d: d.__setitem__(1, 49 * 22 + 15)):
        data, d, _ = FR.record_frame(rng, 50, 22)
        d = d.copy()
        edit(d)
        bad.append((data + bytes(300 * 50), d, np.zeros((50, 4), np.float32)))
    frames = [goods[0]] + bad[:3] + [goods[1]] + bad[3:] + [goods[2]]
    chunk, desc, offs, want = FR.build_chunk(frames, lead=1)
    for d in desc:      # what a refused descriptor names by off and step lies inside the chunk
        for c in range(4):
            if 1 <= d[11 + c] <= 8:
                assert 0 <= d[0] + d[3 + c] and d[0] + d[3 + c] + 49 * d[7 + c] + 8 <= chunk.size
    rows, status = run_into(env, chunk, desc, offs, tail=4096)
    assert status.tolist() == [0] + [FR.E_LAYOUT] * 3 + [0] + [FR.E_LAYOUT] * 5 + [0]
    assert np.array_equal(bits(rows), bits(want))
    # a span that does not lie inside the chunk
    d = goods[0][1].copy()
    d[1] += 1
    rows, _, status = run(env, np.frombuffer(goods[0][0], np.uint8), d[None], tail=4096)
    assert status.tolist() == [FR.E_LAYOUT] and not bits(rows).any()


def test_unpack_front_end(env):
    pf, dev = env["pf"], env["dev"]
    rows, offs, status = pf.unpack(torch.zeros(0, dtype=torch.uint8, device=dev), [])
    assert tuple(rows.shape) == (0, 4) and offs.cpu().tolist() == [0] and status.numel() == 0
    data, d, want = FR.record_frame(np.random.default_rng(16), 100, 22)
    chunk = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(dev)
    out = torch.full((130, 4), -1.0, device=dev)
    rows, _, status = pf.unpack(chunk, [d], out=out)
    torch.cuda.synchronize()
    assert rows.data_ptr() == out.data_ptr() and np.array_equal(bits(rows.cpu().numpy()), bits(want)) and bool((out[100:] == -1).all())
    with pytest.raises(ValueError, match="out must be"):
        pf.unpack(chunk, [d], out=torch.empty((99, 4), device=dev))
    with pytest.raises(ValueError, match="flat uint8"):
        pf.unpack(chunk.view(-1, 2), [d])
