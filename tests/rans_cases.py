"""The case table of the 'rans' format, shared by the reference's, the host build's and the GPU tests.

valid()     name -> (data, width, chunk_log2): what the encoders are given.  chunk_log2 is 8 unless the name says otherwise.  With 256-byte
            chunks a chunk's state flush (4 bytes for each of its min(64, k) lanes) is as long as the chunk, so every such case takes the
            stored form; the coded form is reached by the same contents at chunk_log2 9, 10 and 12 ('c9_' ...), by the case at the default
            chunk size and by the example sweep's arrays.
forced()    name -> (stream, data): the coded form of every case of valid() with n > 0, stored fallback off (rans_ref.encode(fallback=False)):
            what the decoders read, so that they meet chunks of 1 .. 256 bytes, partial last rounds and three chunks within 515 bytes.
golden()    the four arrays of tests/golden/example_64E.npz as its container carries them -> name -> (data, width).
hostile()   name -> (stream, dst_cap), built from BASE: all 256 symbols present (so a flipped symbol byte always breaks the table's order),
            515 bytes in three chunks."""
import bz2
import functools
import os
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import rans_ref as R  # noqa: E402

LENGTHS = (0, 1, 3, 63, 64, 65, 255, 256, 257, 2 * 256 + 3)
WIDTHS = (1, 2, 4)


def _contents(rng, n):
    """name -> n bytes."""
    out = {}
    out["one"] = bytes([7]) * n
    out["two"] = bytes(np.where(rng.random(n) < 0.8, 3, 200).astype(np.uint8))
    dom = np.full(n, 9, np.uint8)                       # one dominant symbol, the 255 others once each where n allows
    rare = np.array([s for s in range(256) if s != 9], np.uint8)[: max(n - 1, 0)]
    dom[rng.permutation(n)[: rare.size]] = rare
    out["dominant"] = bytes(dom)
    out["even"] = bytes(np.resize(np.arange(256, dtype=np.uint8), n))
    out["random"] = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    out["int16"] = np.rint(rng.normal(0, 3, n // 2 + 1)).astype("<i2").tobytes()[:n]      # high bytes 0x00 / 0xFF: one plane nearly constant
    rows = np.tile(np.array([0.6, -0.3, 0.74, 1.7], "<f4"), (n // 16 + 1, 1)) + rng.normal(0, 1e-3, (n // 16 + 1, 4)).astype("<f4")
    out["float32"] = rows.astype("<f4").tobytes()[:n]
    return out


_NATURAL = {"int16": 2, "float32": 4}   # the contents that belong to one width


@functools.lru_cache(maxsize=None)
def valid():
    rng = np.random.default_rng(19)
    out = {}
    for n in LENGTHS:
        for name, data in _contents(rng, n).items():
            for w in WIDTHS:
                if _NATURAL.get(name, w) == w or n in (3, 257):
                    out["%s_n%d_w%d" % (name, n, w)] = (data, w, 8)
    for clog, n in ((9, 2 * 512 + 3), (10, 2 * 1024 + 65), (10, 1000), (12, 3 * 4096 + 5)):   # (the last: rare symbols raised to 1)
        for name, data in _contents(rng, n).items():
            for w in WIDTHS:
                if _NATURAL.get(name, w) == w:
                    out["c%d_%s_n%d_w%d" % (clog, name, n, w)] = (data, w, clog)
    n = 2 * (1 << R.DEFAULT_CHUNK_LOG2) + 1001            # the default chunk size, 3 chunks
    out["default_int16_n%d_w2" % n] = (_contents(rng, n)["int16"], 2, R.DEFAULT_CHUNK_LOG2)
    return out


@functools.lru_cache(maxsize=None)
def golden():
    blob = np.load(os.path.join(HERE, "golden", "example_64E.npz"))["rpcc"].tobytes()
    out, off = {}, 0
    for k, w in (("contour_map", 1), ("idx_sequence", 2), ("plane_param", 4), ("residual_quantized", 2)):
        (n,) = struct.unpack_from("i", blob, off)
        out[k] = (bz2.decompress(blob[off + 4: off + 4 + n]), w)
        off += 4 + n
    assert off == len(blob)
    return out


@functools.lru_cache(maxsize=None)
def everything():
    """valid() and golden() (at the default chunk size): name -> (data, width, chunk_log2), every stream the pins cover."""
    out = dict(valid())
    out.update({"golden_" + k: (d, w, R.DEFAULT_CHUNK_LOG2) for k, (d, w) in golden().items()})
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    return R.encode(*everything()[name])


@functools.lru_cache(maxsize=None)
def forced():
    return {name: (R.encode(d, w, c, fallback=False), d) for name, (d, w, c) in valid().items() if len(d) and c < R.DEFAULT_CHUNK_LOG2}


@functools.lru_cache(maxsize=None)
def base():
    """(stream, data, (end of header, end of tables, end of directory)) of the hostile streams' origin."""
    data, w, c = valid()["dominant_n515_w1"]
    s = R.encode(data, w, c, fallback=False)
    st, info = R.parse(s, len(data))
    assert st == R.OK and s[12:14] == struct.pack("<H", 256)
    spans = info[5]
    assert len(spans) == 3 and len({l for _, l in spans}) > 1
    return s, data, (12, 12 + 2 + 3 * 256, spans[0][0])


def _flip(s, k):
    b = bytearray(s)
    b[k >> 3] ^= 1 << (k & 7)
    return bytes(b)


@functools.lru_cache(maxsize=None)
def hostile():
    s, data, (h, t, d) = base()
    cap = len(data)
    out = {}
    for k in range(8 * d):                               # every single-bit flip of header, table and directory
        out["flip_%s_%d" % ("header" if k < 8 * h else "table" if k < 8 * t else "directory", k)] = (_flip(s, k), cap)
    for k in range(len(s)):
        out["cut_%d" % k] = (s[:k], cap)
    out["appended"] = (s + b"\0", cap)
    lens = list(struct.unpack_from("<3I", s, t))
    out["directory_exchanged"] = (s[:t] + struct.pack("<3I", lens[2], lens[1], lens[0]) + s[d:], cap)
    e = 14 + 3 * 9                                       # the dominant symbol's entry; its neighbours have frequency 1
    (g,), (f,) = struct.unpack_from("<H", s, e - 2), struct.unpack_from("<H", s, e + 1)
    assert s[e] == 9 and f > 16
    out["freq_sum_kept"] = (s[: e - 2] + struct.pack("<H", g + 1) + s[e: e + 1] + struct.pack("<H", f - 1) + s[e + 3:], cap)   # one from 9 to 8
    out["freq_sum_changed"] = (s[: e + 1] + struct.pack("<H", f - 1) + s[e + 3:], cap)
    w = d + 4 * 64 + 2                                   # the second word of the first chunk
    out["payload_word_flipped"] = (_flip(s, 8 * w + 3), cap)
    out["n_above_capacity"] = (s, cap - 1)
    out["stored_n_above_capacity"] = (R.encode(data, 1, 8), cap - 1)
    out["stored_cut"] = (R.encode(data, 1, 8)[:-1], cap)
    out["stored_appended"] = (R.encode(data, 1, 8) + b"\0", cap)
    out["coded_n0"] = (R.header(1, 1, 0, 8) + struct.pack("<H", 0), 0)
    return out
