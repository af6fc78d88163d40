"""Reference of the device inflate (include/rpcc_inflate.h) in plain Python: one gzip member, then nothing
or zero bytes, decoded with exactly the statuses of rpcc_inflate_decode.  The status is the first check that fails in stream
order; gzip.decompress accepts exactly the streams that are OK here (tests/test_inflate_ref.py), but for a second member.

A Huffman symbol is read bit by bit (canonical codes, shortest first): E_TRUNCATED when the input ends before a code matches,
E_SYMBOL when 15 bits match none."""
import struct
import zlib

OK, E_TRUNCATED, E_HEADER, E_BTYPE, E_STORED, E_TABLE, E_SYMBOL, E_OFFSET, E_OVERRUN, E_CRC, E_SIZE, E_TRAILING = \
    0, -2, -3, -4, -5, -6, -7, -8, -9, -10, -11, -12
NAMES = {OK: "OK", E_TRUNCATED: "E_TRUNCATED", E_HEADER: "E_HEADER", E_BTYPE: "E_BTYPE", E_STORED: "E_STORED", E_TABLE: "E_TABLE",
         E_SYMBOL: "E_SYMBOL", E_OFFSET: "E_OFFSET", E_OVERRUN: "E_OVERRUN", E_CRC: "E_CRC", E_SIZE: "E_SIZE", E_TRAILING: "E_TRAILING"}

LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
CODES, LENS, DISTS = 0, 1, 2


class _Stop(Exception):
    def __init__(self, status):
        self.status = status


class _Bits:
    def __init__(self, data, pos):
        self.d, self.pos, self.bit = data, pos, 0     # next bit: bit `bit` of d[pos]

    def left(self):
        return 8 * (len(self.d) - self.pos) - self.bit

    def take(self, n):
        if n > self.left():
            raise _Stop(E_TRUNCATED)
        v = 0
        for k in range(n):
            v |= ((self.d[self.pos] >> self.bit) & 1) << k
            self.bit += 1
            if self.bit == 8:
                self.bit, self.pos = 0, self.pos + 1
        return v

    def align(self):
        if self.bit:
            self.bit, self.pos = 0, self.pos + 1


def _table(lens, kind):
    """zlib's rules for a set of code lengths -> (count per length, symbols sorted by (length, symbol))."""
    count = [0] * 16
    for x in lens:
        count[x] += 1
    count[0] = 0
    left = 1
    for b in range(1, 16):
        left = 2 * left - count[b]
        if left < 0:
            raise _Stop(E_TABLE)                      # over-subscribed
    mx = max([b for b in range(1, 16) if count[b]], default=0)
    if left > 0 and (kind == CODES or (mx != 1 and mx != 0) or (mx == 0 and kind != DISTS)):
        raise _Stop(E_TABLE)                          # incomplete
    return count, [s for b in range(1, 16) for s, x in enumerate(lens) if x == b]


def _symbol(br, tab, rep=None):
    count, order = tab
    code = first = index = 0
    for b in range(1, 16):
        code |= br.take(1)
        if code - count[b] < first:
            if rep is not None:
                rep["max_code_length"] = max(rep["max_code_length"], b)
            return order[index + code - first]
        index += count[b]
        first = (first + count[b]) << 1
        code <<= 1
    raise _Stop(E_SYMBOL)


_FIXED = None


def _fixed():
    global _FIXED
    if _FIXED is None:
        _FIXED = (_table([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, LENS), _table([5] * 32, DISTS))
    return _FIXED


def inflate(data, cap=None, report=False):
    """-> (status, bytes produced) [, report]: data is one stream of rpcc_inflate_decode, cap its dst_cap (None: no limit)."""
    data = bytes(data)
    out = bytearray()
    rep = {"blocks": [], "max_code_length": 0, "max_distance": 0, "min_match": None, "max_match": None, "far_match": 0}
    try:
        _member(data, out, cap, rep)
        st = OK
    except _Stop as e:
        st = e.status
    return (st, bytes(out), rep) if report else (st, bytes(out))


def _member(d, out, cap, rep):
    n = len(d)
    if n == 0:
        return
    pos = 0

    def need(k):
        if pos + k > n:
            raise _Stop(E_TRUNCATED)

    need(2)
    if d[0] != 0x1F or d[1] != 0x8B:
        raise _Stop(E_HEADER)
    need(3)
    if d[2] != 8:
        raise _Stop(E_HEADER)
    need(10)
    flg = d[3]
    pos = 10
    if flg & 4:
        need(2)
        xlen = d[pos] | d[pos + 1] << 8
        pos += 2
        need(xlen)
        pos += xlen
    for bit in (8, 16):
        if flg & bit:
            while True:
                need(1)
                pos += 1
                if d[pos - 1] == 0:
                    break
    if flg & 2:
        need(2)
        pos += 2
    br = _Bits(d, pos)
    room = (lambda: 1 << 62) if cap is None else (lambda: cap - len(out))
    while True:
        final = br.take(1)
        btype = br.take(2)
        rep["blocks"].append(btype)
        if btype == 3:
            raise _Stop(E_BTYPE)
        if btype == 0:
            br.align()
            ln = br.take(16)
            nl = br.take(16)
            if ln != (~nl & 0xFFFF):
                raise _Stop(E_STORED)
            if ln > n - br.pos:
                raise _Stop(E_TRUNCATED)
            if ln > room():
                raise _Stop(E_OVERRUN)
            out += d[br.pos: br.pos + ln]
            br.pos += ln
        else:
            if btype == 1:
                lt, dt = _fixed()
            else:
                hlit, hdist, hclen = br.take(5) + 257, br.take(5) + 1, br.take(4) + 4
                if hlit > 286 or hdist > 30:
                    raise _Stop(E_TABLE)
                cl = [0] * 19
                for k in range(hclen):
                    cl[CL_ORDER[k]] = br.take(3)
                ct = _table(cl, CODES)
                lens = []
                while len(lens) < hlit + hdist:
                    s = _symbol(br, ct)
                    if s < 16:
                        lens.append(s)
                        continue
                    if s == 16:
                        if not lens:
                            raise _Stop(E_TABLE)
                        v, r = lens[-1], 3 + br.take(2)
                    elif s == 17:
                        v, r = 0, 3 + br.take(3)
                    else:
                        v, r = 0, 11 + br.take(7)
                    if len(lens) + r > hlit + hdist:
                        raise _Stop(E_TABLE)
                    lens += [v] * r
                if lens[256] == 0:
                    raise _Stop(E_TABLE)
                lt = _table(lens[:hlit], LENS)
                dt = _table(lens[hlit:], DISTS)
            while True:
                s = _symbol(br, lt, rep)
                if s < 256:
                    if room() < 1:
                        raise _Stop(E_OVERRUN)
                    out.append(s)
                    continue
                if s == 256:
                    break
                if s > 285:
                    raise _Stop(E_SYMBOL)
                ln = LEN_BASE[s - 257] + br.take(LEN_EXTRA[s - 257])
                ds = _symbol(br, dt, rep)
                if ds > 29:
                    raise _Stop(E_SYMBOL)
                dist = DIST_BASE[ds] + br.take(DIST_EXTRA[ds])
                if dist > len(out):
                    raise _Stop(E_OFFSET)
                if ln > room():
                    raise _Stop(E_OVERRUN)
                if dist >= rep["max_distance"]:       # far_match: the longest match at the largest distance
                    rep["far_match"] = ln if dist > rep["max_distance"] else max(rep["far_match"], ln)
                rep["max_distance"] = max(rep["max_distance"], dist)
                rep["min_match"] = ln if rep["min_match"] is None else min(rep["min_match"], ln)
                rep["max_match"] = ln if rep["max_match"] is None else max(rep["max_match"], ln)
                if dist >= ln:
                    out += out[len(out) - dist: len(out) - dist + ln]
                else:
                    seg = bytes(out[len(out) - dist:])
                    out += (seg * (ln // dist + 1))[:ln]
        if final:
            break
    br.align()
    pos = br.pos
    need(8)
    crc, isize = struct.unpack_from("<II", d, pos)
    if crc != zlib.crc32(out):
        raise _Stop(E_CRC)
    if isize != len(out) & 0xFFFFFFFF:
        raise _Stop(E_SIZE)
    if any(d[pos + 8:]):
        raise _Stop(E_TRAILING)
