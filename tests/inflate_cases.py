"""Streams of the inflate tests (tests/test_inflate_ref.py on the CPU, tests/test_gpu_inflate.py on the GPU), built on the CPU once
per process; every stream is seeded.

valid()      name -> (stream, the bytes it decodes to, check(report)): each case says through inflate_ref's report what it is there for
flips()      every single-bit flip of four small members         truncations()  every proper prefix of one, but the empty one
hand_built() name -> (stream, dst_cap, status): one stream per status and per table rule, written with a small bit writer
many_lane()  [(name, stream, dst_cap)]: the part of all these that the 64-thread host build runs (tests/test_inflate_core_host.py)"""
import functools
import gzip
import io
import os
import struct
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import deflate_cases  # noqa: E402
import deflate_ref  # noqa: E402
import inflate_ref as R  # noqa: E402

STORED, FIXED, DYNAMIC = 0, 1, 2


def _z(data, level=6, mem=8, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, 31, mem, strategy)
    return c.compress(bytes(data)) + c.flush()


def _blocks(kind, lo, hi=None):
    hi = lo if hi is None else hi

    def check(rep):
        assert set(rep["blocks"]) == {kind} and lo <= len(rep["blocks"]) <= hi, rep["blocks"]
    return check


def _match(distance, length):
    def check(rep):
        assert rep["max_distance"] == distance and rep["max_match"] == length, rep
    return check


def _far(distance):
    """A match of 258 bytes at this distance, the largest of the stream: every lane of a copy step takes part at it."""
    def check(rep):
        assert rep["max_distance"] == distance and rep["max_match"] == 258 and rep["far_match"] >= 64, rep
    return check


def _any(rep):
    pass


def _turns(plain, turns):
    def check(rep):
        assert len(plain) // 32768 >= turns
    return check


@functools.lru_cache(maxsize=None)
def valid():
    rng = np.random.default_rng(11)
    out = {}
    for n in (0, 1):
        src = bytes(range(65, 65 + n))
        out["gzip_n%d" % n] = (gzip.compress(src, mtime=0), src, _blocks(FIXED, 1))
        out["ref_n%d" % n] = (deflate_ref.compress(src), src, _blocks(STORED, 1))
    for n, nb in ((65535, 1), (65536, 2), (70000, 2)):      # (zlib may end a stream with one more, empty, stored block)
        src = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        out["level0_%d" % n] = (_z(src, 0), src, _blocks(STORED, nb, nb + 1))
    src = deflate_cases.edge_inputs()["random_65535"]
    out["ref_stored_65535"] = (deflate_cases.reference("random_65535"), src, _blocks(STORED, 1))     # LEN = 65535
    src = rng.integers(0, 4, 3000, dtype=np.uint8).tobytes()
    out["fixed"] = (_z(src, 6, 8, zlib.Z_FIXED), src, _blocks(FIXED, 1))
    src = np.rint(rng.normal(0, 3, 1500)).astype(np.int16).tobytes()
    out["dynamic_blocks"] = (_z(src, 9, 1), src, _blocks(DYNAMIC, 3, 100))
    src = rng.integers(0, 256, 3000, dtype=np.uint8).tobytes()
    out["stored_blocks"] = (_z(src, 1, 1), src, _blocks(STORED, 3, 100))
    fib = [1, 1]
    while len(fib) < 20:
        fib.append(fib[-1] + fib[-2])
    src = rng.permutation(np.repeat(np.arange(20, dtype=np.uint8), fib)).tobytes()
    assert len(src) == 17710

    def fifteen(rep):
        assert rep["max_code_length"] == 15, rep
    out["fibonacci"] = (_z(src, 6, 8, zlib.Z_HUFFMAN_ONLY), src, fifteen)
    src = bytes(300000)
    out["zeros_zlib"] = (_z(src), src, _match(1, 258))
    out["zeros_ref"] = (deflate_ref.compress(src), src, _match(1, 258))
    src = deflate_cases.far_pattern(32768)
    out["far_32768"] = (deflate_ref.compress(src), src, _match(32768, 258))   # zlib itself stops at 32506
    # at 32768 every lane of a copy step reads the ring slot it fills itself; at 32705 .. 32767 it reads one that another lane fills in
    # the same step (lane + 32768 - distance), so the step's loads must all come before its stores; 32704 is the last distance without
    for d in (32704, 32705, 32737, 32767):
        src = deflate_cases.far_pattern(d, 258)
        out["far_%d" % d] = (deflate_ref.compress(src), src, _far(d))
    # short distances with whole-wave matches: the copy's periodic branch (k < P) below, at and above the wave's 64 lanes
    for d in (2, 3, 63, 64, 65):
        src = (rng.integers(1, 256, d, dtype=np.uint8).tobytes() * (700 // d + 2))[:700]
        out["near_%d" % d] = (deflate_ref.compress(src), src, _far(d))
    # 4100 periodic bytes, then 200 random ones: the byte that fills a piece of 4160 is a literal, stored by one lane just before the flush
    src = (rng.integers(1, 256, 7, dtype=np.uint8).tobytes() * 600)[:4100] + rng.integers(0, 256, 200, dtype=np.uint8).tobytes()

    def literal_fills_the_piece(rep):
        assert rep["max_distance"] == 7 and set(rep["blocks"]) <= {FIXED, DYNAMIC}, rep
    out["flush_at_literal"] = (_z(src, 9), src, literal_fills_the_piece)
    for name, a in deflate_cases.golden_arrays().items():
        src = np.ascontiguousarray(a).tobytes()
        chk = _turns(src, 5) if len(src) == 188106 else _any
        out["golden_zlib_" + name] = (gzip.compress(src, mtime=0), src, chk)
        out["golden_ref_" + name] = (deflate_cases.reference(name), src, chk)
    assert any(len(p) == 188106 for _, p, _ in out.values())      # the residuals turn the ring over five times
    buf = io.BytesIO()
    src = b"a member with a file name " * 9
    with gzip.GzipFile("sweep_0001.bin", "wb", 6, buf, mtime=0) as f:
        f.write(src)

    def named(rep):
        assert buf.getvalue()[3] & 8
    out["file_name"] = (buf.getvalue(), src, named)
    out["zero_padded"] = (_z(src) + bytes(3), src, _any)
    return out


@functools.lru_cache(maxsize=None)
def small_members():
    """Four members of a few hundred bytes, one per block type and encoder -> [(stream, plain)]."""
    rng = np.random.default_rng(12)
    src = (np.rint(rng.normal(0, 2, 150)).astype(np.int16).tobytes() + b"the same words, the same words, and the same words again. " * 3)
    return [(_z(src, 9), src), (_z(src, 6, 8, zlib.Z_FIXED), src), (_z(src[:200], 0), src[:200]),
            (deflate_ref.compress(src), src)]


@functools.lru_cache(maxsize=None)
def flips():
    """-> [(stream, dst_cap)]: every single-bit flip of small_members(); dst_cap is the original's size."""
    out = []
    for m, plain in small_members():
        for k in range(8 * len(m)):
            b = bytearray(m)
            b[k >> 3] ^= 1 << (k & 7)
            out.append((bytes(b), len(plain)))
    return out


@functools.lru_cache(maxsize=None)
def truncations():
    m, plain = small_members()[0]
    return [(m[:k], len(plain)) for k in range(1, len(m))]


# The many-lane host run costs two thread barriers for every symbol, so it takes the streams of at most MANY_LANE_STREAM bytes (the far
# matches are among them: 40000 bytes from 468), those of MANY_LANE_STORED (a stored byte costs no barrier, and only a stored block of
# more than a piece flushes inside its own loop) and every MANY_LANE_STRIDE-th flip and truncation.
MANY_LANE_STREAM = 2048
MANY_LANE_STORED = ("level0_65536", "stored_blocks")
MANY_LANE_STRIDE = 211


def many_lane():
    rows = [(name, s, cap) for name, (s, cap, _) in hand_built().items()] + [("empty", b"", 0)]
    rows += [(name, s, len(p)) for name, (s, p, _) in valid().items() if len(s) <= MANY_LANE_STREAM or name in MANY_LANE_STORED]
    rows += [("flip%d" % k, s, cap) for k, (s, cap) in list(enumerate(flips()))[::MANY_LANE_STRIDE]]
    rows += [("cut%d" % k, s, cap) for k, (s, cap) in list(enumerate(truncations()))[::MANY_LANE_STRIDE // 8]]
    return rows


class Bits:
    """LSB-first bit writer."""

    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, value, bits):
        self.v |= (value & ((1 << bits) - 1)) << self.n
        self.n += bits
        return self

    def code(self, code, bits):
        """A Huffman code, given most significant bit first as RFC 1951 states it."""
        return self.put(int(format(code, "0%db" % bits)[::-1], 2), bits)

    def align(self):
        self.n = (self.n + 7) // 8 * 8
        return self

    def bytes(self):
        return self.align().v.to_bytes(self.n // 8, "little")


def member(body, plain=b""):
    return deflate_ref.HEADER + body + struct.pack("<II", zlib.crc32(plain), len(plain))


def fixed_lit(bw, s):
    if s < 144:
        return bw.code(0x30 + s, 8)
    if s < 256:
        return bw.code(0x190 + s - 144, 9)
    if s < 280:
        return bw.code(s - 256, 7)
    return bw.code(0xC0 + s - 280, 8)


_CL = [4] * 13 + [5] * 6      # a complete code-length code over all 19 symbols


def dynamic_header(bw, lit, dist, hlit=None, hdist=None):
    """BFINAL = 1, BTYPE = 2 and the code lengths lit + dist, one code-length symbol each (no repeats)."""
    cc = deflate_ref.canonical_codes(_CL)
    bw.put(1, 1).put(2, 2).put((len(lit) if hlit is None else hlit) - 257, 5).put((len(dist) if hdist is None else hdist) - 1, 5).put(15, 4)
    for s in R.CL_ORDER:
        bw.put(_CL[s], 3)
    for x in list(lit) + list(dist):
        bw.put(cc[x], _CL[x])
    return bw


def _cl_header(bw, hlit, hdist, cl):
    """BFINAL = 1, BTYPE = 2 and a code-length code given as {symbol: length} -> the symbols' codes (LSB first)."""
    lens = [cl.get(s, 0) for s in range(19)]
    hclen = max(4, max(k for k in range(19) if lens[R.CL_ORDER[k]]) + 1)
    bw.put(1, 1).put(2, 2).put(hlit - 257, 5).put(hdist - 1, 5).put(hclen - 4, 4)
    for k in range(hclen):
        bw.put(lens[R.CL_ORDER[k]], 3)
    return lens


def _lit3():
    """Literal 'a' in 1 bit, 256 and 257 in 2 bits: a complete code.  -> (lengths [258], codes)"""
    lit = [0] * 258
    lit[97], lit[256], lit[257] = 1, 2, 2
    return lit, deflate_ref.canonical_codes(lit)


@functools.lru_cache(maxsize=None)
def hand_built():
    out = {}
    pad = bytes(8)
    out["btype_3"] = (member(Bits().put(1, 1).put(3, 2).bytes()), 0, R.E_BTYPE)
    out["len_nlen"] = (member(Bits().put(1, 1).put(0, 2).align().put(5, 16).put(5, 16).bytes() + b"hello", b"hello"), 5, R.E_STORED)
    out["hlit_30"] = (member(Bits().put(1, 1).put(2, 2).put(30, 5).put(0, 5).put(0, 4).bytes() + pad), 0, R.E_TABLE)
    out["hdist_31"] = (member(Bits().put(1, 1).put(2, 2).put(0, 5).put(30, 5).put(0, 4).bytes() + pad), 0, R.E_TABLE)
    bw = Bits()
    _cl_header(bw, 257, 1, {16: 1, 17: 1, 18: 1})
    out["code_lengths_oversubscribed"] = (member(bw.bytes() + pad), 0, R.E_TABLE)
    bw = Bits()
    _cl_header(bw, 257, 1, {16: 1})
    out["code_lengths_incomplete"] = (member(bw.bytes() + pad), 0, R.E_TABLE)
    bw = Bits()
    _cl_header(bw, 257, 1, {0: 1, 16: 1})            # 0 -> '0', 16 -> '1'
    out["repeat_first"] = (member(bw.put(1, 1).put(0, 2).bytes() + pad), 0, R.E_TABLE)
    bw = Bits()
    _cl_header(bw, 257, 1, {0: 1, 18: 1})            # 0 -> '0', 18 -> '1'
    out["repeat_past_end"] = (member(bw.put(1, 1).put(127, 7).put(1, 1).put(127, 7).bytes() + pad), 0, R.E_TABLE)
    bw = Bits()
    _cl_header(bw, 257, 1, {1: 1, 18: 1})            # 1 -> '0', 18 -> '1': lengths 1, 1, then 256 zeros
    out["no_end_of_block"] = (member(bw.put(0, 1).put(0, 1).put(1, 1).put(127, 7).put(1, 1).put(107, 7).bytes() + pad), 0, R.E_TABLE)
    lit = [0] * 258
    lit[97], lit[256] = 2, 2                          # half of the code space unused
    out["literals_incomplete"] = (member(dynamic_header(Bits(), lit, [1]).bytes() + pad), 0, R.E_TABLE)
    lit[97], lit[256], lit[257] = 1, 1, 1
    out["literals_oversubscribed"] = (member(dynamic_header(Bits(), lit, [1]).bytes() + pad), 0, R.E_TABLE)
    lit, lc = _lit3()
    out["distances_oversubscribed"] = (member(dynamic_header(Bits(), lit, [1, 1, 1]).bytes() + pad), 0, R.E_TABLE)
    out["distances_incomplete"] = (member(dynamic_header(Bits(), lit, [2, 2]).bytes() + pad), 0, R.E_TABLE)
    out["literal_286"] = (member(fixed_lit(Bits().put(1, 1).put(1, 2), 286).bytes() + pad), 0, R.E_SYMBOL)
    bw = fixed_lit(fixed_lit(Bits().put(1, 1).put(1, 2), 97), 257).code(30, 5)
    out["distance_30"] = (member(bw.bytes() + pad, b"a"), 4, R.E_SYMBOL)
    bw = fixed_lit(fixed_lit(Bits().put(1, 1).put(1, 2), 97), 257).code(1, 5)      # length 3 at distance 2 after one byte
    out["distance_past_output"] = (member(fixed_lit(bw, 256).bytes(), b"aaaa"), 4, R.E_OFFSET)
    plain = b"capacity " * 30
    out["one_byte_over"] = (_z(plain), len(plain) - 1, R.E_OVERRUN)
    out["exact_capacity"] = (_z(plain), len(plain), R.OK)
    m = bytearray(_z(plain))
    m[-8] ^= 1
    out["wrong_crc"] = (bytes(m), len(plain), R.E_CRC)
    m = bytearray(_z(plain))
    m[-4] ^= 1
    out["wrong_isize"] = (bytes(m), len(plain), R.E_SIZE)
    out["trailing_byte"] = (_z(plain) + b"\0\1", len(plain), R.E_TRAILING)
    out["two_members"] = (_z(plain) + _z(plain), 2 * len(plain), R.E_TRAILING)
    # 'a' 'a' 'a', length 3 at distance 1, end of block; the distance code is one code of one bit ('0')
    bw = dynamic_header(Bits(), lit, [1])
    for s in (97, 97, 97, 257):
        bw.put(lc[s], lit[s])
    out["one_distance_code"] = (member(bw.put(0, 1).put(lc[256], lit[256]).bytes(), b"aaaaaa"), 6, R.OK)
    bw = dynamic_header(Bits(), lit, [1])
    for s in (97, 97, 97, 257):
        bw.put(lc[s], lit[s])
    out["one_distance_code_other_bit"] = (member(bw.put(0xFFFF, 16).bytes() + pad, b"aaaaaa"), 6, R.E_SYMBOL)
    bw = dynamic_header(Bits(), lit, [0])
    bw.put(lc[97], lit[97]).put(lc[256], lit[256])
    out["no_distance_code_unused"] = (member(bw.bytes(), b"a"), 1, R.OK)
    bw = dynamic_header(Bits(), lit, [0])
    bw.put(lc[97], lit[97]).put(lc[257], lit[257])
    out["no_distance_code_needed"] = (member(bw.bytes() + pad, b"a"), 4, R.E_SYMBOL)
    only = [0] * 257
    only[256] = 1                                     # the literal/length code's only code has length 1
    out["only_end_of_block"] = (member(dynamic_header(Bits(), only, [0]).put(0, 1).bytes()), 0, R.OK)
    return out


def gzip_accepts(stream):
    """(True, bytes) where gzip.decompress returns, else (False, None)."""
    try:
        return True, gzip.decompress(stream)
    except (OSError, EOFError, zlib.error, struct.error):
        return False, None
