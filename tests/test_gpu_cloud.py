"""-m gpu: the cloud packer (librpcc_cloud.so, cloud.py) against tests/cloud_ref.py by bits, at the smallest shapes where it can go wrong:
P around the 4096-point round and across three rounds, extra capacities 0, 1 and past one and two rounds, per-frame counts 0, 1, the
capacity, above it (clamped), negative (0) and around the round, B past one trip of a workgroup over the counts; every frame pattern of
tests/rows_cases.py in the pixel segment crossed with all / none / mixed kept in the extra segment; with and without intensity and ri_rec;
rows of exactly `total` rows between guards from a 0xFF and a 0x00 fill; a capacity one row short; two calls chained through `base`; and,
without an extra segment, rows.pack's output."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import buffer_arena as BA  # noqa: E402
import cloud_cases as CC  # noqa: E402
import cloud_ref as C  # noqa: E402
import rows_cases as RC  # noqa: E402

CAPS = (0, 1, 4097, 8193)
KINDS = ("zero", "one", "full", "above", "negative", "half", 4095, 4096, 4097)


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    import rpcc_amd  # noqa: F401
    from rpcc_amd import _cloud_lib, cloud, rows
    assert _cloud_lib.ROUND == 4096           # the shapes below sit around it
    return dict(torch=torch, cl=_cloud_lib, cloud=cloud, rows=rows, dev=torch.device("cuda:0"))


def _dev(env, a):
    return None if a is None else env["torch"].from_numpy(np.ascontiguousarray(a)).to(env["dev"])


def _bits(t):
    return t.detach().cpu().contiguous().numpy().reshape(-1).view(np.uint8)


def _guarded_extra(env, extra):
    """The extra points in an allocation of exactly their bytes, between guards."""
    B, cap, _ = extra.shape
    arena = BA.Arena(max(12 * B * cap, 4), env["dev"], back=1 << 12)
    view = arena.view[: 12 * B * cap].view(env["torch"].float32).view(B, cap, 3)
    view.copy_(_dev(env, extra))
    return arena, view


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("P", [1, 3, 4095, 4096, 4097, 8193])
def test_kernel_equals_reference_by_bits(env, B, P):
    torch, cloud, cl = env["torch"], env["cloud"], env["cl"]
    bounds = (256, 4096, 8192)          # a wavefront's last point | first of the next; a round's last | first of the next
    words = cl.table_words(B)
    table = BA.Arena(8 * words, env["dev"], back=1 << 12)
    nz = BA.Arena(4 * B, env["dev"], back=1 << 12)
    seen_kinds, seen_split, k = set(), set(), 0
    for cap in CAPS:
        for pattern in RC.PATTERNS:
            pc, w, ri = RC.batch(B, P, pattern, boundaries=bounds, seed=3)
            d_pc = _dev(env, pc)
            for epattern in CC.EXTRA_PATTERNS if cap else ("mixed",):
                kind = KINDS[k % len(KINDS)]
                k += 1
                seen_kinds.add(kind)
                counts = CC.counts_for(B, cap, kind)
                extra = CC.extras(B, cap, epattern, counts, boundaries=bounds, seed=k)
                ex_arena, d_ex = _guarded_extra(env, extra) if cap else (None, None)
                d_cnt = _dev(env, counts) if cap else None
                combos = [(True, True), (False, False)] + ([(True, False), (False, True)] if pattern == epattern == "mixed" else [])
                for with_w, with_ri in combos:
                    offsets, want, nonzero = C.pack_batch(pc, w if with_w else None, ri if with_ri else None, extra if cap else None, counts)
                    total = int(offsets[-1])
                    heads = np.diff(C.pack_batch(pc)[0])
                    seen_split.update((bool(h), bool(t)) for h, t in zip(heads, np.diff(offsets) - heads))
                    d_w, d_ri = _dev(env, w if with_w else None), _dev(env, ri if with_ri else None)
                    arena = BA.Arena(max(16 * total, 16), env["dev"], back=1 << 14)
                    out = arena.view[: 16 * total].view(torch.float32).view(total, 4)
                    tag = (B, P, cap, pattern, epattern, kind, with_w, with_ri)
                    for fill in ("ones", "zero"):                      # the same buffers twice, whatever they held: the result repeats
                        arena.fill(fill), table.fill(fill), nz.fill(fill)
                        t, r, n = cloud.pack(d_pc, d_w, d_ri, extra=d_ex, extra_count=d_cnt, rows=out, table=table.view.view(torch.int64),
                                             nonzero=nz.view.view(torch.int32))
                        torch.cuda.synchronize()
                        assert arena.check_guards() is None and table.check_guards() is None and nz.check_guards() is None, (tag, fill)
                        assert ex_arena is None or ex_arena.check_guards() is None, (tag, fill)
                        tab = t.cpu().numpy()
                        assert tab[: B + 1].tolist() == offsets.tolist() and tab[B + 1] == cl.OK, (tag, fill)
                        assert tab[B + 2:].tolist() == np.diff(offsets).tolist(), (tag, fill)
                        bad = np.flatnonzero(_bits(r) != want.reshape(-1).view(np.uint8))
                        assert bad.size == 0, (tag, fill, bad.size, bad[:6])
                        if total == 0:
                            assert (arena.view == (0xFF if fill == "ones" else 0)).all(), (tag, fill)      # nothing kept: nothing written
                        if with_ri:
                            assert n.cpu().numpy().tolist() == nonzero.tolist(), (tag, fill)
                        else:
                            assert n is None and _bits(nz.view).tolist() == ([0xFF] * (4 * B) if fill == "ones" else [0] * (4 * B)), (tag, fill)
                    if total and with_w == with_ri:
                        # a capacity one row short: rows untouched, the true offsets, the status set
                        short = BA.Arena(max(16 * (total - 1), 16), env["dev"], back=1 << 14).fill("ones")
                        small = short.view[: 16 * (total - 1)].view(torch.float32).view(total - 1, 4)
                        t, _, _ = cloud.pack(d_pc, d_w, d_ri, extra=d_ex, extra_count=d_cnt, rows=small)
                        torch.cuda.synchronize()
                        tab = t.cpu().numpy()
                        assert tab[: B + 1].tolist() == offsets.tolist() and tab[B + 1] == cl.E_CAPACITY, tag
                        assert short.check_guards() is None and bool((short.view == 0xFF).all()), tag
    assert seen_kinds == set(KINDS)
    # a frame with no pixel kept and extras kept, the reverse, both and neither
    assert seen_split == {(False, False), (False, True), (True, False), (True, True)}
    # the default buffers: B * (P + capacity) rows always suffice
    cap = 4097
    pc, w, ri = RC.batch(B, P, "all_kept", seed=4)
    counts = np.full(B, cap, np.int32)
    extra = CC.extras(B, cap, "all_kept", counts, seed=4)
    t, r, n = cloud.pack(_dev(env, pc).view(B, 1, P, 3), _dev(env, w).view(B, 1, P), _dev(env, ri).view(B, 1, P), extra=_dev(env, extra), extra_count=_dev(env, counts))
    offsets, want, nonzero = C.pack_batch(pc, w, ri, extra, counts)
    assert r.shape == (B * (P + cap), 4) and int(offsets[-1]) == B * (P + cap) and t.cpu().numpy()[: B + 2].tolist() == offsets.tolist() + [cl.OK]
    assert np.array_equal(_bits(r), want.reshape(-1).view(np.uint8)) and n.cpu().numpy().tolist() == nonzero.tolist()


def test_hostile_table_in_both_segments(env):
    torch, cloud = env["torch"], env["cloud"]
    n = len(RC.HOSTILE)
    pc, w = RC.hostile_pc()[None], RC.hostile_w()[None]
    extra = np.concatenate([RC.hostile_pc()[::-1], np.full((2, 3), CC.POISON, np.float32)])[None]
    for count in (n, n + 2, n + 50, 0, -1):
        counts = np.array([count], np.int32)
        offsets, want, _ = C.pack_batch(pc, w, None, extra, counts)
        t, r, _ = cloud.pack(_dev(env, pc), _dev(env, w), extra=_dev(env, extra), extra_count=_dev(env, counts))
        torch.cuda.synchronize()
        assert t.cpu().numpy()[:2].tolist() == offsets.tolist(), count
        got = r[: int(offsets[-1])].cpu().numpy()
        assert got.view(np.uint32).tobytes() == want.view(np.uint32).tobytes(), count
    kept = int(RC.hostile_kept().sum())
    assert np.isnan(got[:kept, :3]).any() and not got.view(np.uint32)[kept:, 3].any()       # (count -1: the pixel rows alone)


def test_many_frames(env):
    """B = 1025: one more than a workgroup's trip over the counts of the frames before it."""
    torch, cloud, cl = env["torch"], env["cloud"], env["cl"]
    B, P, cap = 1025, 3, 5
    pc, w, ri = RC.batch(B, P, "mixed", seed=6)
    pc[1024], pc[1023] = (1.0, 2.0, 3.0), 0
    rng = np.random.default_rng(8)
    counts = rng.integers(-2, cap + 3, B).astype(np.int32)
    counts[-1], counts[0] = cap, 1
    extra = CC.extras(B, cap, "mixed", counts, seed=6)
    offsets, want, nonzero = C.pack_batch(pc, w, ri, extra, counts)
    total = int(offsets[-1])
    arena = BA.Arena(16 * total, env["dev"], back=1 << 14).fill("ones")
    out = arena.view.view(torch.float32).view(total, 4)
    t, r, n = cloud.pack(_dev(env, pc), _dev(env, w), _dev(env, ri), extra=_dev(env, extra), extra_count=_dev(env, counts), rows=out)
    torch.cuda.synchronize()
    tab = t.cpu().numpy()
    assert arena.check_guards() is None
    assert tab[: B + 1].tolist() == offsets.tolist() and tab[B + 1] == cl.OK and n.cpu().numpy().tolist() == nonzero.tolist()
    assert np.array_equal(_bits(r), want.reshape(-1).view(np.uint8))
    assert offsets[1025] - offsets[1024] >= 3 and len(set(np.diff(offsets).tolist())) > 4


def test_calls_chained_through_base(env):
    """Two calls into one rows buffer, the second starting where the first ended without the host knowing where: the batch's rows, and a
    capacity that the two together exceed is reported by the second call alone."""
    torch, cloud, cl = env["torch"], env["cloud"], env["cl"]
    P, cap = 4096 + 77, 4097
    pc, w, ri = RC.batch(5, P, "empty_middle", boundaries=(256, 4096), seed=9)
    counts = CC.counts_for(5, cap, "half")
    extra = CC.extras(5, cap, "mixed", counts, boundaries=(256, 4096), seed=9)
    offsets, want, nonzero = C.pack_batch(pc, w, ri, extra, counts)
    total = int(offsets[-1])
    dv = lambda a: _dev(env, a)
    for room, status in ((total, cl.OK), (total - 1, cl.E_CAPACITY)):
        arena = BA.Arena(16 * room, env["dev"], back=1 << 14).fill("ones")
        out = arena.view.view(torch.float32).view(room, 4)
        t1, _, n1 = cloud.pack(dv(pc[:2]), dv(w[:2]), dv(ri[:2]), extra=dv(extra[:2]), extra_count=dv(counts[:2]), rows=out)
        t2, _, n2 = cloud.pack(dv(pc[2:]), dv(w[2:]), dv(ri[2:]), extra=dv(extra[2:]), extra_count=dv(counts[2:]), rows=out, base=t1[2:3])
        torch.cuda.synchronize()
        a, b = t1.cpu().numpy(), t2.cpu().numpy()
        assert a[:3].tolist() == offsets[:3].tolist() and a[3] == cl.OK
        assert b[:4].tolist() == offsets[2:].tolist() and b[4] == status
        assert n1.cpu().numpy().tolist() + n2.cpu().numpy().tolist() == nonzero.tolist()
        assert arena.check_guards() is None
        first = int(offsets[2])
        assert np.array_equal(_bits(out[:first]), want[:first].reshape(-1).view(np.uint8))
        if status == cl.OK:
            assert np.array_equal(_bits(out), want.reshape(-1).view(np.uint8))
        else:
            assert bool((arena.view[16 * first:] == 0xFF).all())


@pytest.mark.parametrize("P", [3, 4097, 8193])
def test_without_extras_equals_the_row_packer(env, P):
    torch, cloud, rows = env["torch"], env["cloud"], env["rows"]
    for B, pattern in ((1, "mixed"), (3, "empty_first"), (3, "all_kept")):
        pc, w, ri = RC.batch(B, P, pattern, boundaries=(256, 4096, 8192), seed=12)
        d = [_dev(env, a) for a in (pc, w, ri)]
        want = rows.pack(*d, rows=BA.filled((B * P, 4), torch.float32, env["dev"], 0xEE))
        zero_cap = torch.empty((B, 0, 3), dtype=torch.float32, device=env["dev"])
        ignored = BA.filled((B, 9, 3), torch.float32, env["dev"], 0x3F)          # points of counts that are all <= 0
        for kw in (dict(), dict(extra=zero_cap, extra_count=_dev(env, np.full(B, 7, np.int32))),
                   dict(extra=ignored, extra_count=_dev(env, np.array([0, -1, -(2 ** 31)][:B], np.int32)))):
            got = cloud.pack(*d, rows=BA.filled((B * P, 4), torch.float32, env["dev"], 0xEE), **kw)
            torch.cuda.synchronize()
            for a, b in zip(got, want):
                assert np.array_equal(_bits(a), _bits(b)), (P, B, pattern, sorted(kw))
