"""The case table of version 2 of the 'rans' format (the delta filter), shared by the reference's, the host build's
and the GPU tests.  Small shapes only: 512- and 1024-byte chunks, so that several chunks, the reset at a chunk's first element and the
carry from one 256-byte block of the decoder's scan to the next are all reached within a few KB.

valid()     name -> (data, width, chunk_log2, filter): what the encoders are given.  Contents (elements of `width` bytes):
              walk    a random walk of steps -2 .. 2 around a large value: compressible only through the filter, and every chunk's first
                      element is large (prev = 0 there)
              zeros   all zero: one symbol in every table
              equal   one non-zero value: the chunk's first element and zeros
              ramp    a constant step
              alt     the lowest and the highest signed value in turn (int16: -32768 / 32767): every difference wraps
              half    0 and 2^(8 width - 1) in turn (width 4: steps of 0x80000000)
              random  incompressible: the stored fallback
            at 63, 64, 65, chunk - width, chunk, chunk + width and 2 chunk + 1 bytes for chunk_log2 9 and 10, at 0, 1, width - 1, width
            and width + 1 bytes, and a few unfiltered (filter 0) cases to mix with them.
forced()    name -> (stream, data): the 'RB' form of every filtered case with n > 0, fallback off -- what the decoders read.
hostile()   name -> (stream, dst_cap) from BASE, a three-chunk 'RB' stream."""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import rans_filter_ref as F  # noqa: E402
import rans_ref as R  # noqa: E402

WIDTHS = (1, 2, 4)
CHUNK_LOG2 = (9, 10)


def lengths(width, clog):
    chunk = 1 << clog
    return (63, 64, 65, chunk - width, chunk, chunk + width, 2 * chunk + 1)


def _contents(rng, n, width):
    """name -> n bytes (the last n % width of them a cut element)."""
    e = n // width + 1
    dt, bits = "<u%d" % width, 8 * width
    big = (1 << (bits - 1)) - (1 << (bits - 3))                       # 0x60, 0x6000, 0x60000000
    cut = lambda a: np.asarray(a).astype(np.uint64).astype(dt).tobytes()[:n]
    out = {}
    out["walk"] = cut((big + np.cumsum(rng.integers(-2, 3, e))) % (1 << bits))
    out["zeros"] = bytes(n)
    out["equal"] = cut(np.full(e, big + 5))
    out["ramp"] = cut((np.arange(e, dtype=np.uint64) * 3 + 7) % (1 << bits))
    out["alt"] = cut(np.where(np.arange(e) % 2 == 0, 1 << (bits - 1), (1 << (bits - 1)) - 1))     # as signed: lowest, highest
    out["half"] = cut(np.where(np.arange(e) % 2 == 0, 0, 1 << (bits - 1)))
    out["random"] = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    return out


@functools.lru_cache(maxsize=None)
def valid():
    rng = np.random.default_rng(192)
    out = {}
    for clog in CHUNK_LOG2:
        for w in WIDTHS:
            for n in lengths(w, clog):
                for name, data in _contents(rng, n, w).items():
                    out["c%d_%s_n%d_w%d" % (clog, name, n, w)] = (data, w, clog, F.FILTER_DELTA)
    for w in WIDTHS:
        for n in sorted({0, 1, w - 1, w, w + 1}):
            out["c9_walk_n%d_w%d" % (n, w)] = (_contents(rng, n, w)["walk"], w, 9, F.FILTER_DELTA)
    for w in WIDTHS:                                                   # the same contents without the filter, to mix into one call
        out["c10_plain_n2049_w%d" % w] = (_contents(rng, 2049, w)["walk"], w, 10, F.FILTER_NONE)
        out["c10_plainzeros_n1024_w%d" % w] = (bytes(1024), w, 10, F.FILTER_NONE)
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    d, w, c, f = valid()[name]
    return F.encode(d, w, c, f)


@functools.lru_cache(maxsize=None)
def forced():
    return {name: (F.encode(d, w, c, f, fallback=False), d) for name, (d, w, c, f) in valid().items() if len(d) and f == F.FILTER_DELTA}


@functools.lru_cache(maxsize=None)
def base():
    """(stream, data) of the hostile streams' origin: three chunks of 512 bytes, width 2, coded."""
    data, w, c, f = valid()["c9_walk_n1025_w2"]
    s = F.encode(data, w, c, f)
    assert s[:2] == b"RB" and s == forced()["c9_walk_n1025_w2"][0] and F.parse(s, len(data))[0] == F.OK
    return s, data


def _flip(s, k):
    b = bytearray(s)
    b[k >> 3] ^= 1 << (k & 7)
    return bytes(b)


def _with(s, at, value):
    b = bytearray(s)
    b[at] = value
    return bytes(b)


@functools.lru_cache(maxsize=None)
def hostile():
    s, data = base()
    cap = len(data)
    out = {}
    for k in range(8 * R.HEADER):                          # every single-bit flip of the header
        out["flip_header_%d" % k] = (_flip(s, k), cap)
    out["filter_0"] = (_with(s, 9, 0), cap)
    out["filter_2"] = (_with(s, 9, 2), cap)
    out["filter_255"] = (_with(s, 9, 255), cap)
    out["mode_0"] = (_with(s, 2, 0), cap)
    out["mode_0_stored_length"] = (_with(s, 2, 0)[: R.HEADER] + data, cap)          # what a stored 'RB' stream would be: there is none
    out["reserved_10"] = (_with(s, 10, 1), cap)
    out["reserved_11"] = (_with(s, 11, 0x80), cap)
    out["n_0"] = (s[:4] + bytes(4) + s[8:], cap)
    for k in range(len(s)):
        out["cut_%d" % k] = (s[:k], cap)
    out["appended"] = (s + b"\0", cap)
    out["appended_2"] = (s + b"\0\0", cap)
    out["payload_bit"] = (_flip(s, 8 * (len(s) - 3) + 2), cap)
    out["n_above_capacity"] = (s, cap - 1)
    out["version_1_magic"] = (b"RA" + s[2:], cap)         # an 'RA' header with byte 9 set is refused as before
    return out
