"""Test helper for the caller-buffer contract of the libraries (include/*.h): workspaces of EXACTLY the size a `*_bytes` function
returns, filled with hostile contents and surrounded by guard bytes the test owns, and a way to list the output bytes a call leaves alone.

torch only; works on CPU tensors (tests/test_buffer_arena.py) and on the GPU (tests/test_gpu_buffers.py)."""
import re

import torch

ALIGN = 256
GUARD_BYTE = 0xA5          # the guards' content: no pattern below fills whole words with it

# 32-bit words of the named patterns (word i of the view): see fill()
_CONST = {"zero": 0x00000000, "ones": 0xFFFFFFFF, "intmax": 0x7FFFFFFF, "nan": 0x7FC00000}
PATTERNS = tuple(_CONST) + tuple("alt(%d,%d)" % (s, p) for s in (0, 1, 2) for p in (0, 1)) + ("half(0)", "half(1)")
_ALT = re.compile(r"^alt\((\d+),\s*(\d+)\)$")
_HALF = re.compile(r"^half\(([01])\)$")


def pattern_words(pattern, n, device="cpu"):
    """The first n 32-bit words of `pattern` as an int32 tensor (two's complement of the unsigned value).
    zero / ones (a word read as a counter is -1, so a mark `word + 1` is 0) / intmax (`word + 1` wraps) / nan (a quiet NaN for
    areas read as floats) / alt(s,p): word i = 1000 + (((i >> s) & 1) ^ p) -- whichever word a kernel takes for a running mark,
    under one of the two parities p half of the words at stride 2^s hold mark + 1.
    half(p): word i = 0 where (i & 1) == p, 0xFFFFFFFF elsewhere -- a cleared word next to a dirty one.  Every other pattern is all zero or
    has no zero word at all, so a kernel that takes a non-zero flag word for "use the slow exact path" would hide a table it forgot to clear;
    under one parity the flag reads 0 while the 64-bit sums beside it (and one half of every 32-bit table) hold garbage."""
    if pattern in _CONST:
        v = _CONST[pattern]
        return torch.full((n,), v - (1 << 32) if v >= 1 << 31 else v, dtype=torch.int32, device=device)
    h = _HALF.match(pattern)
    if h:
        i = torch.arange(n, dtype=torch.int64, device=device)
        return (((i & 1) ^ int(h.group(1))) * -1).to(torch.int32)
    m = _ALT.match(pattern)
    if not m:
        raise ValueError("unknown pattern %r (one of %s)" % (pattern, ", ".join(PATTERNS)))
    s, p = int(m.group(1)), int(m.group(2))
    i = torch.arange(n, dtype=torch.int64, device=device)
    return (1000 + (((i >> s) & 1) ^ p)).to(torch.int32)


class Arena:
    """One uint8 allocation: [ slack | front guard | view of exactly nbytes bytes, 256-byte aligned | back guard ]."""

    def __init__(self, nbytes, device="cpu", front=4096, back=1 << 20):
        self.nbytes, self.front, self.back = int(nbytes), int(front), int(back)
        assert self.nbytes > 0 and self.front >= 0 and self.back >= 0
        self.raw = torch.empty(self.front + self.nbytes + self.back + ALIGN, dtype=torch.uint8, device=device)
        self.start = (-(self.raw.data_ptr() + self.front)) % ALIGN + self.front      # offset of the view inside raw
        self.view = self.raw[self.start: self.start + self.nbytes]
        assert self.view.data_ptr() % ALIGN == 0 and self.view.numel() == self.nbytes
        self._front = self.raw[self.start - self.front: self.start]
        self._back = self.raw[self.start + self.nbytes: self.start + self.nbytes + self.back]
        self.fill("zero")

    def first(self, n):
        """The view's first n bytes (a smaller workspace at the same address; the rest of the view then acts as more guard)."""
        assert 0 <= n <= self.nbytes, (n, self.nbytes)
        return self.view[:n]

    def fill(self, pattern):
        """Guards to GUARD_BYTE, the view to `pattern` (a trailing part word gets the leading bytes of its word, little endian)."""
        self.raw.fill_(GUARD_BYTE)
        nw = (self.nbytes + 3) // 4
        if nw:
            w = pattern_words(pattern, nw, self.raw.device).view(torch.uint8)
            self.view.copy_(w[: self.nbytes])
        return self

    def check_guards(self):
        """None when no guard byte changed; else (lowest, highest) changed offset relative to the view's first byte (negative: in
        front of it; >= nbytes: behind it)."""
        lo = hi = None
        for g, base in ((self._front, -self.front), (self._back, self.nbytes)):
            bad = torch.nonzero(g != GUARD_BYTE).flatten()
            if bad.numel():
                a, b = base + int(bad[0]), base + int(bad[-1])
                lo = a if lo is None else min(lo, a)
                hi = b if hi is None else max(hi, b)
        return None if lo is None else (lo, hi)


def unwritten(run, outputs=None):
    """run(fill_byte) -> {name: tensor}: the outputs of one call whose output buffers were all pre-filled with fill_byte (run does
    the filling: it owns the allocation).  Called with 0x00 and 0xFF.  -> {name: bool tensor over the output's BYTES, flat, True =
    the two runs differ there = the call did not write that byte}.  A byte that IS written holds the same value in both runs, so
    equal bytes also show that the call repeats itself exactly.  outputs (a dict): receives the outputs of the 0x00 run."""
    a = {k: v.detach().clone() for k, v in run(0x00).items()}
    b = run(0xFF)
    assert a.keys() == b.keys()
    if outputs is not None:
        outputs.update(a)
    holes = {}
    for k in a:
        x, y = a[k].contiguous().reshape(-1).view(torch.uint8), b[k].contiguous().reshape(-1).view(torch.uint8)
        assert x.shape == y.shape, k
        holes[k] = x != y
    return holes


def filled(shape, dtype, device, fill_byte):
    """A tensor whose every byte is fill_byte."""
    t = torch.empty(shape, dtype=dtype, device=device)
    t.reshape(-1).view(torch.uint8).fill_(fill_byte)
    return t
