"""Streams of the bunzip2 tests (tests/test_bunzip2_ref.py and tests/test_bunzip2_core_host.py on the CPU, tests/test_gpu_bunzip2.py on
the GPU), built on the CPU once per process; every stream is seeded.

valid()        name -> (stream, the bytes it decodes to)        golden_members()  the four arrays of tests/golden/example_64E.npz
flips()        every single-bit flip of small_stream()          truncations()     every proper prefix of it but the empty one
hand_built()   name -> (stream, dst_cap, nblock_max, status): one stream per rule, written with a small bit writer and block encoder
FLIP_CAP, FLIP_BLOCK: the capacity and work-slot block length the flips and truncations are decoded with.
many_lane()    [(name, stream, dst_cap, work block length)]: the part of all these that the 64-thread host build runs"""
import bz2
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import bunzip2_ref as R  # noqa: E402

FLIP_CAP, FLIP_BLOCK = 65536, 100000


@functools.lru_cache(maxsize=None)
def golden_members():
    """name -> bzip2 stream, in the container's order."""
    import struct
    blob = np.load(os.path.join(HERE, "golden", "example_64E.npz"))["rpcc"].tobytes()
    out, off = {}, 0
    for k in ("contour_map", "idx_sequence", "plane_param", "residual_quantized"):
        (n,) = struct.unpack_from("i", blob, off)
        out[k] = blob[off + 4: off + 4 + n]
        off += 4 + n
    assert off == len(blob) and all(v[:4] == b"BZh9" for v in out.values())
    return out


@functools.lru_cache(maxsize=None)
def valid():
    rng = np.random.default_rng(21)
    out = {}
    for n in (0, 1, 4, 5):
        out["len%d" % n] = bytes(range(65, 65 + n))
    for n in (4, 5, 255, 256, 259, 260):
        out["run%d" % n] = b"x" + b"r" * n + b"y"
    out["count_equals_byte"] = b"\x04" * 8 + b"z" + b"\x00" * 4 + b"\x05" * 9      # 4 x 04 then count 04; 4 x 00 then count 00; 4 x 05 then count 05
    out["zeros70000"] = bytes(70000)
    out["all_bytes"] = bytes(range(256)) * 3
    out["two_symbols"] = rng.integers(0, 2, 5000, dtype=np.uint8).tobytes()
    out["abc_period"] = b"abc" * 2000
    rnd = rng.integers(0, 50, 250000, dtype=np.uint8).tobytes()
    res = {k: (bz2.compress(v), v) for k, v in out.items()}
    res["random_level1"] = (bz2.compress(rnd, 1), rnd)
    res["random_level9"] = (bz2.compress(rnd, 9), rnd)
    for k, m in golden_members().items():
        res["golden_" + k] = (m, bz2.decompress(m))
    return res


@functools.lru_cache(maxsize=None)
def small_stream():
    """One stream of about 150 bytes -> (stream, plain)."""
    rng = np.random.default_rng(22)
    plain = np.rint(rng.normal(0, 2, 90)).astype(np.int16).tobytes() + b"the same words, " * 3 + b"\0" * 9
    s = bz2.compress(plain)
    assert 130 <= len(s) <= 180, len(s)
    return s, plain


@functools.lru_cache(maxsize=None)
def flips():
    s, _ = small_stream()
    out = []
    for k in range(8 * len(s)):
        b = bytearray(s)
        b[k >> 3] ^= 0x80 >> (k & 7)
        out.append(bytes(b))
    return out


@functools.lru_cache(maxsize=None)
def truncations():
    s, _ = small_stream()
    return [s[:k] for k in range(1, len(s))]


# The many-lane host run (tests/test_bunzip2_core_host.py) costs a dozen thread barriers for every symbol, so it takes the valid streams
# of at most MANY_LANE_STREAM bytes and every MANY_LANE_STRIDE-th flip and truncation.
MANY_LANE_STREAM = 512
MANY_LANE_STRIDE = 97


def many_lane():
    rows = [(name, s, cap, slot) for name, (s, cap, slot, _) in hand_built().items()] + [("empty", b"", 0, 0)]
    rows += [(name, s, len(p), R.block_bound(int(s[3:4]), len(p))) for name, (s, p) in valid().items() if len(s) <= MANY_LANE_STREAM]
    rows += [("flip%d" % k, s, FLIP_CAP, FLIP_BLOCK) for k, s in list(enumerate(flips()))[::MANY_LANE_STRIDE]]
    rows += [("cut%d" % k, s, FLIP_CAP, FLIP_BLOCK) for k, s in list(enumerate(truncations()))[::MANY_LANE_STRIDE // 8]]
    return rows


# ---- a small bzip2 writer
class Bits:
    """MSB-first bit writer."""

    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, value, bits):
        self.v = self.v << bits | (value & ((1 << bits) - 1))
        self.n += bits
        return self

    def bytes(self):
        pad = -self.n % 8
        return (self.v << pad).to_bytes((self.n + pad) // 8, "big")


def rle1(plain):
    """bzip2's first run-length stage: four equal bytes, then a count of 0..255 more."""
    out, i = bytearray(), 0
    while i < len(plain):
        j = i
        while j < len(plain) and plain[j] == plain[i] and j - i < 259:
            j += 1
        n = j - i
        out += plain[i: i + min(n, 4)]
        if n >= 4:
            out.append(n - 4)
        i = j
    return bytes(out)


def bwt(pre):
    n = len(pre)
    rot = sorted(range(n), key=lambda i: pre[i:] + pre[:i])
    return bytes(pre[i - 1] for i in rot), rot.index(0)


def run_symbols(r):
    out = []
    while r > 0:
        if r & 1:
            out.append(0)
            r = (r - 1) >> 1
        else:
            out.append(1)
            r = (r - 2) >> 1
    return out


def mtf_symbols(ll, seq):
    mtf, syms, run = list(seq), [], 0
    for b in ll:
        j = mtf.index(b)
        if j == 0:
            run += 1
            continue
        syms += run_symbols(run)
        run = 0
        syms.append(j + 1)
        mtf.insert(0, mtf.pop(j))
    return syms + run_symbols(run) + [len(seq) + 1]


def assign_codes(lens):
    """libbz2's BZ2_hbAssignCodes."""
    codes, vec = [0] * len(lens), 0
    for n in range(min(lens), max(lens) + 1):
        for i, x in enumerate(lens):
            if x == n:
                codes[i] = vec
                vec += 1
        vec <<= 1
    return codes


def flat_lengths(alpha):
    """A complete prefix code over alpha symbols."""
    k = max(1, (alpha - 1).bit_length())
    short = (1 << k) - alpha
    return [k - 1] * short + [k] * (alpha - short) if k > 1 else [1] * alpha


def block(bw, pre, seq=None, lens=None, ngroups=2, selectors=None, sel_raw=None, nsel=None, orig=None, rnd=0, crc=None, syms=None,
          codes=None, plain=None, first_len=None):
    """One block of the pre-RLE1 bytes `pre` into bw -> the block's CRC.  Every field can be overridden."""
    ll, o = bwt(pre) if pre else (b"", 0)
    seq = sorted(set(pre)) if seq is None else seq
    alpha = len(seq) + 2
    syms = mtf_symbols(ll, seq) if syms is None else syms
    lens = [flat_lengths(alpha)] * ngroups if lens is None else lens
    if plain is None:
        plain = R.unrle(pre) or b""
    have = (R.crc(plain) ^ 0xFFFFFFFF) if crc is None else crc
    bw.put(R.BLOCK_MAGIC, 48).put(have, 32).put(rnd, 1).put(o if orig is None else orig, 24)
    used = [sum(1 << (15 - k) for k in range(16) if 16 * i + k in seq) for i in range(16)]
    bw.put(sum(1 << (15 - i) for i in range(16) if used[i]), 16)
    for u in used:
        if u:
            bw.put(u, 16)
    bw.put(ngroups, 3)
    count = -(-len(syms) // R.GROUP)
    selectors = [0] * count if selectors is None else selectors
    bw.put(len(selectors) if nsel is None else nsel, 15)
    if sel_raw is None:
        order, sel_raw = list(range(6)), []
        for s in selectors:
            j = order.index(s)
            sel_raw.append(j)
            order.insert(0, order.pop(j))
    for j in sel_raw:
        bw.put((1 << (j + 1)) - 2, j + 1)
    for t in lens:
        curr = t[0] if first_len is None else first_len
        bw.put(curr, 5)
        for x in t:
            while curr != x:
                bw.put(2 if x > curr else 3, 2)
                curr += 1 if x > curr else -1
            bw.put(0, 1)
    for k, s in enumerate(syms):
        t = selectors[k // R.GROUP] if k // R.GROUP < len(selectors) else 0
        if codes is not None:
            c, n = codes[s]
        else:
            c, n = assign_codes(lens[t])[s], lens[t][s]
        bw.put(c, n)
    return have


def stream(blocks, level=9, combined=None, magic=b"BZh", end=R.END_MAGIC):
    """blocks: [(pre, options)] -> one stream."""
    bw = Bits()
    for ch in magic:
        bw.put(ch, 8)
    bw.put(0x30 + level, 8)
    comb = 0
    for pre, opt in blocks:
        have = block(bw, pre, **opt)
        comb = ((comb << 1 | comb >> 31) & 0xFFFFFFFF) ^ have
    bw.put(end, 48).put(comb if combined is None else combined, 32)
    return bw.bytes()


def _text(n, letters, seed):
    rng = np.random.default_rng(seed)
    return bytes(rng.choice(np.frombuffer(letters, np.uint8), n))


@functools.lru_cache(maxsize=None)
def hand_built():
    """name -> (stream, dst_cap, nblock_max, status)."""
    BIG, SLOT = 1 << 16, 100000
    out = {}

    def add(name, s, status, cap=BIG, slot=SLOT):
        out[name] = (s, cap, slot, status)

    words = _text(400, b"abcdefg", 1)
    text = rle1(words)                                        # the blocks below are given as pre-RLE1 bytes
    add("tables_2", stream([(text, {})]), R.OK)
    six = [flat_lengths(9)] * 2 + [[2, 3, 3, 3, 3, 4, 4, 4, 4]] * 2 + [[4, 4, 4, 4, 3, 3, 3, 3, 2]] * 2
    nsym = len(mtf_symbols(bwt(text)[0], sorted(set(text))))
    add("tables_6", stream([(text, {"ngroups": 6, "lens": six, "selectors": [k % 6 for k in range(-(-nsym // 50))]})]), R.OK)
    add("tables_6_all_selected_last", stream([(text, {"ngroups": 6, "lens": six, "selectors": [5] * -(-nsym // 50)})]), R.OK)
    add("three_blocks", stream([(text, {}), (text[:50], {}), (b"q", {})], level=1), R.OK)
    add("no_blocks", stream([]), R.OK, cap=0, slot=0)
    letters = bytes(range(97, 97 + 19))                       # 21 symbols: lengths 1 .. 19, 20, 20 are a complete code
    deep = letters * 3 + _text(200, letters, 2)
    add("code_20_bits", stream([(deep, {"lens": [list(range(1, 20)) + [20, 20]] * 2})]), R.OK)
    one = b"\x07"
    # two byte values in use; symbol 2 and the end of block in one bit each, the two run symbols in two: over-subscribed.  The rule reads
    # one bit and never a second, so '0' '1' is symbol 2, end of block.
    over = {"seq": [7, 9], "lens": [[2, 2, 1, 1]] * 2, "syms": [2, 3], "codes": {2: (0, 1), 3: (1, 1)}, "orig": 0, "plain": b"\x09"}
    add("oversubscribed", stream([(one, over)]), R.OK)
    add("incomplete", stream([(text, {"lens": [[x + 1 for x in flat_lengths(9)]] * 2})]), R.OK)
    hole = {"seq": [7, 9], "lens": [[3, 3, 3, 3]] * 2, "syms": [2, 3], "codes": {2: (7, 3), 3: (3, 3)}, "orig": 0, "plain": b"\x09"}
    add("incomplete_hole", stream([(one, hole)]) + bytes(4), R.E_SYMBOL)
    add("selector_past_groups", stream([(text, {"sel_raw": [0, 2] + [0] * (-(-nsym // 50) - 2)})]), R.E_TABLE)
    add("selectors_none", stream([(text, {"nsel": 0, "sel_raw": []})]), R.E_TABLE)
    add("selectors_too_few", stream([(text, {"selectors": [0] * (-(-nsym // 50) - 1)})]) + bytes(8), None)
    many = [0] * 18010
    add("selectors_18010", stream([(text, {"selectors": many})]), R.OK)
    add("groups_1", stream([(text, {"ngroups": 1})]), R.E_TABLE)
    add("groups_7", stream([(text, {"ngroups": 7, "lens": [flat_lengths(9)] * 7})]), R.E_TABLE)
    add("length_0", stream([(text, {"first_len": 0})]), R.E_TABLE)
    add("length_21", stream([(text, {"first_len": 21})]), R.E_TABLE)
    add("empty_symbol_map", stream([(text, {"seq": [], "syms": [0], "lens": [[1, 1]] * 2})]), R.E_TABLE)
    add("origin_equals_length", stream([(text, {"orig": len(text)})]), R.E_ORIGPTR)
    add("origin_last", stream([(text, {"orig": len(text) - 1})]), None)
    add("origin_huge", stream([(text, {"orig": 900011})]), R.E_ORIGPTR)
    add("origin_900010", stream([(text, {"orig": 900010})]), R.E_ORIGPTR)
    run = {"seq": [7], "syms": run_symbols(100001) + [2], "plain": b""}
    add("run_past_block_limit", stream([(one, run)], level=1), R.E_SYMBOL)
    run = {"seq": [7], "syms": run_symbols(100000) + [2], "plain": b"", "crc": 0}
    add("run_to_block_limit", stream([(one, run)], level=1), None, slot=100000)
    add("run_past_slot", stream([(one, run)], level=2), R.E_WORK, slot=99999)
    run = {"seq": [7], "syms": [1] * 22 + [2], "plain": b""}
    add("run_overflow", stream([(one, run)]), R.E_SYMBOL)
    add("randomised", stream([(text, {"rnd": 1})]), R.E_RANDOMISED)
    good = stream([(text, {})])
    add("second_stream", good + good, R.E_TRAILING)
    add("trailing_zeros", good + bytes(3), R.E_TRAILING)
    add("trailing_partial_stream", good + b"BZ", R.E_TRAILING)
    add("block_crc", stream([(text, {"crc": 12345})]), R.E_CRC)
    add("combined_crc", stream([(text, {})], combined=1), R.E_CRC)
    add("bad_block_magic", stream([(text, {})], end=R.END_MAGIC ^ 1), R.E_MAGIC)
    add("level_0", stream([(text, {})], level=0), R.E_HEADER)
    add("magic_BZx", stream([(text, {})], magic=b"BZx"), R.E_HEADER)
    four = b"ab" + b"c" * 4
    add("four_equal_then_end", stream([(four, {"plain": four})]), R.E_RLE)
    add("four_equal_count_then_end", stream([(four + b"\x02", {})]), R.OK)
    add("count_byte_is_run_byte", stream([(b"k" + b"\x03" * 5 + b"\x03" * 4 + b"\x00", {})]), R.OK)
    add("one_byte_over", good, R.E_OVERRUN, cap=len(words) - 1)
    add("exact_capacity", good, R.OK, cap=len(words))
    add("slot_exact", good, R.OK, slot=len(text))
    add("slot_one_short", good, R.E_WORK, slot=len(text) - 1)
    add("overrun_then_bad_crc", stream([(text, {}), (text, {"crc": 5})]), R.E_CRC, cap=10)
    return out


def bz2_accepts(s):
    """(True, bytes) where bz2.decompress returns, else (False, None)."""
    try:
        return True, bz2.decompress(s)
    except (OSError, ValueError, EOFError):
        return False, None
