"""The buffer-contract helper itself (tests/buffer_arena.py) on CPU tensors: what the GPU tests rely on must hold before they run."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from buffer_arena import ALIGN, GUARD_BYTE, PATTERNS, Arena, filled, pattern_words, unwritten   # noqa: E402


@pytest.mark.parametrize("nbytes", [1, 3, 4, 255, 256, 257, 4099, 100001])
def test_view_is_aligned_exact_and_guarded(nbytes):
    a = Arena(nbytes, "cpu", front=512, back=1024)
    assert a.view.data_ptr() % ALIGN == 0
    assert a.view.numel() == nbytes and a.view.dtype == torch.uint8          # no rounding up
    half = a.first((nbytes + 1) // 2)
    assert half.data_ptr() == a.view.data_ptr() and half.numel() == (nbytes + 1) // 2
    raw0 = a.raw.data_ptr()
    assert a.view.data_ptr() - raw0 >= 512                                   # the whole front guard lies inside the allocation
    assert a.view.data_ptr() - raw0 + nbytes + 1024 <= a.raw.numel()         # ... and the back guard
    assert a._front.numel() == 512 and a._back.numel() == 1024
    assert a._front.data_ptr() + 512 == a.view.data_ptr() and a._back.data_ptr() == a.view.data_ptr() + nbytes
    assert a.check_guards() is None


def test_pattern_words():
    n = 37
    i = np.arange(n)
    want = {"zero": np.zeros(n, np.uint32), "ones": np.full(n, 0xFFFFFFFF, np.uint32), "intmax": np.full(n, 0x7FFFFFFF, np.uint32),
            "nan": np.full(n, 0x7FC00000, np.uint32)}
    for s in (0, 1, 2):
        for p in (0, 1):
            want["alt(%d,%d)" % (s, p)] = (1000 + (((i >> s) & 1) ^ p)).astype(np.uint32)
    for q in (0, 1):
        want["half(%d)" % q] = np.where((i & 1) == q, 0, 0xFFFFFFFF).astype(np.uint32)
    assert sorted(want) == sorted(PATTERNS)
    for name in PATTERNS:
        assert np.array_equal(pattern_words(name, n).numpy().view(np.uint32), want[name]), name
    assert np.isnan(pattern_words("nan", 4).numpy().view(np.float32)).all()
    assert (pattern_words("ones", 4).numpy() + 1 == 0).all()                                   # epoch = -1: the mark is 0
    assert (pattern_words("intmax", 4).numpy().astype(np.int32) + np.int32(1) < 0).all()      # the mark wraps
    for q in (0, 1):         # an aligned 64-bit word is dirty under both parities while one of its halves reads 0
        w64 = pattern_words("half(%d)" % q, 8).numpy().view(np.int64)
        assert (w64 != 0).all() and (pattern_words("half(%d)" % q, 8).numpy()[q::2] == 0).all()
    with pytest.raises(ValueError):
        pattern_words("alt(0)", 4)
    with pytest.raises(ValueError):
        pattern_words("half(2)", 4)


@pytest.mark.parametrize("s", [0, 1, 2])
def test_alt_forces_the_collision_wherever_the_mark_lives(s):
    """Take ANY word e of the view for the running mark: a word f holds word[e] + 1 under exactly one of the two parities when bit s of
    e and f differ, and under neither otherwise.  So of a flag array stored 2^s words per frame, every second frame collides with the
    mark in one of the two runs -- frames at odd and at even positions both get their turn once e's side is unknown."""
    n = 64
    w = [pattern_words("alt(%d,%d)" % (s, p), n).numpy() for p in (0, 1)]
    for e in range(n):
        for f in range(n):
            hit = [int(w[p][f]) == int(w[p][e]) + 1 for p in (0, 1)]
            differ = ((e >> s) & 1) != ((f >> s) & 1)
            assert any(hit) == differ                     # words on the other side of bit s collide, in exactly one parity
            assert sum(hit) <= 1
        stride = 1 << s
        flags = np.arange(0, n, stride)                   # a flag array stored 2^s words per frame, from an aligned start
        for p in (0, 1):
            eq = w[p][flags] == w[p][e] + 1
            assert eq.sum() in (0, len(flags) // 2)
        assert sum(int((w[p][flags] == w[p][e] + 1).sum()) for p in (0, 1)) == len(flags) // 2


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("nbytes", [4096, 4099, 2])
def test_fill_writes_view_and_guards(pattern, nbytes):
    a = Arena(nbytes, "cpu", front=256, back=512)
    a.view.fill_(0x11)
    a._front.fill_(0x22)
    a._back.fill_(0x33)
    assert a.check_guards() == (-256, nbytes + 511)
    a.fill(pattern)
    assert a.check_guards() is None
    assert (a._front == GUARD_BYTE).all() and (a._back == GUARD_BYTE).all()
    nw = (nbytes + 3) // 4
    want = pattern_words(pattern, nw).numpy().view(np.uint8)[:nbytes]
    assert np.array_equal(a.view.numpy(), want)
    if nbytes >= 4:
        assert np.array_equal(a.view[: nbytes // 4 * 4].view(torch.int32).numpy(), pattern_words(pattern, nbytes // 4).numpy())


def test_a_one_byte_write_in_either_guard_is_found():
    n = 1000
    a = Arena(n, "cpu", front=300, back=700).fill("alt(0,1)")
    assert a.check_guards() is None
    a.view.fill_(0)                                          # writes inside the view are the callee's right
    assert a.check_guards() is None
    for off in (-300, -1):
        a.fill("ones")
        a.raw[a.start + off] = 0
        assert a.check_guards() == (off, off)
    for off in (n, n + 699):
        a.fill("ones")
        a.raw[a.start + off] = 0
        assert a.check_guards() == (off, off)
    a.fill("nan")
    a.raw[a.start - 7] = 1
    a.raw[a.start + n + 40] = 1
    assert a.check_guards() == (-7, n + 40)
    a.fill("zero")
    a.raw[a.start + n] = GUARD_BYTE                          # a write of the guard's own value cannot be seen: the guard byte is
    assert a.check_guards() is None                          # chosen so that no pattern word and no cleared word looks like it


def test_unwritten_finds_a_planted_hole():
    calls = []

    def run(fill_byte):
        calls.append(fill_byte)
        full = filled((4, 8), torch.float32, "cpu", fill_byte)
        full.copy_(torch.arange(32, dtype=torch.float32).reshape(4, 8))
        holed = filled((5, 6), torch.int16, "cpu", fill_byte)
        holed[:, :4] = 7
        holed[2, 1] = -1                                      # 0xFFFF: equals the second fill, but is written in both runs
        return dict(full=full, holed=holed)

    out = {}
    holes = unwritten(run, out)
    assert calls == [0x00, 0xFF]
    assert not holes["full"].any() and holes["full"].numel() == 4 * 8 * 4
    h = holes["holed"].reshape(5, 6, 2)
    assert h[:, 4:].all() and not h[:, :4].any()
    assert torch.equal(out["holed"][:, :4], run(0x55)["holed"][:, :4])
    t = filled((3,), torch.float64, "cpu", 0xFF)
    assert (t.view(torch.uint8) == 0xFF).all()


def test_unwritten_sees_a_call_that_does_not_repeat_itself():
    k = [0]

    def run(fill_byte):
        k[0] += 1
        return dict(x=torch.full((4,), k[0], dtype=torch.int32))

    assert unwritten(run)["x"].any()
