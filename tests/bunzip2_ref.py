"""The device bunzip2 (include/rpcc_bunzip2.h, csrc_bunzip2/bunzip2_core.h) stated in Python: one bzip2 stream ->
(status, bytes, size, src_used).  The rules are libbz2 1.0.8's as bz2.decompress shows them (tests/test_bunzip2_ref.py holds this file to
it): a symbol is what the limit / base / perm rule reads bit by bit from the shortest length, whether or not the lengths are a prefix code.
The bits are read in the same pieces as the kernel reads them, so src_used agrees on every stream, malformed ones included.  numpy only."""
import numpy as np

OK, E_TRUNCATED, E_HEADER, E_MAGIC, E_RANDOMISED, E_TABLE, E_SYMBOL, E_ORIGPTR, E_OVERRUN, E_CRC, E_WORK, E_TRAILING, E_RLE = \
    0, -2, -3, -4, -5, -6, -7, -8, -9, -10, -11, -12, -13
NAMES = {OK: "OK", E_TRUNCATED: "E_TRUNCATED", E_HEADER: "E_HEADER", E_MAGIC: "E_MAGIC", E_RANDOMISED: "E_RANDOMISED", E_TABLE: "E_TABLE",
         E_SYMBOL: "E_SYMBOL", E_ORIGPTR: "E_ORIGPTR", E_OVERRUN: "E_OVERRUN", E_CRC: "E_CRC", E_WORK: "E_WORK", E_TRAILING: "E_TRAILING",
         E_RLE: "E_RLE"}

BLOCK_MAGIC, END_MAGIC = 0x314159265359, 0x177245385090
MAX_SELECTORS, GROUP = 18002, 50
RUN_LIMIT = 2 * 1024 * 1024


def _crc_table():
    t = []
    for i in range(256):
        r = i << 24
        for _ in range(8):
            r = ((r << 1) ^ (0x04C11DB7 if r & 0x80000000 else 0)) & 0xFFFFFFFF
        t.append(r)
    return t


CRC_TABLE = _crc_table()


def crc(data, r=0xFFFFFFFF):
    """bzip2's CRC register over data (most significant bit first); the stored value is its complement."""
    for b in data:
        r = ((r << 8) & 0xFFFFFFFF) ^ CRC_TABLE[(r >> 24) ^ b]
    return r


def work_bytes(nblock_max):
    """rpcc_bunzip2_stream_work_bytes: a 32-bit link and a byte for each position of the largest block."""
    return 5 * max(int(nblock_max), 0)


def block_bound(level, cap):
    """The longest block a stream of this level that decodes to at most cap bytes can hold (rpcc_bunzip2.h)."""
    return min(100000 * level, 5 * cap // 4 + 8)


class _Fail(Exception):
    pass


def decode_tables(lens):
    """libbz2's BZ2_hbCreateDecodeTables -> (minLen, limit, base, perm)."""
    n = len(lens)
    lo, hi = min(lens), max(lens)
    perm = [j for i in range(lo, hi + 1) for j in range(n) if lens[j] == i]
    base = [0] * 23
    for x in lens:
        base[x + 1] += 1
    for i in range(1, 23):
        base[i] += base[i - 1]
    limit = [0] * 23
    vec = 0
    for i in range(lo, hi + 1):
        vec += base[i + 1] - base[i]
        limit[i] = vec - 1
        vec <<= 1
    for i in range(lo + 1, hi + 1):
        base[i] = ((limit[i - 1] + 1) << 1) - base[i]
    return lo, limit, base, perm


def unrle(pre):
    """Inverse of the first run-length stage over one block -> bytes, or None where the block ends after four equal bytes: libbz2 reads the
    count that belongs there from beyond the block and then reports the block as corrupt."""
    out = bytearray()
    c, last = 0, -1
    for b in pre:
        if c == 4:
            out += bytes([last]) * b
            c = 0
            continue
        if c and b == last:
            c += 1
        else:
            c, last = 1, b
        out.append(b)
    return None if c == 4 else bytes(out)


def bunzip2(data, cap=None, nblock_max=None, report=False):
    """One stream -> (status, bytes, size, src_used).  cap: the destination's size (None: any); nblock_max: the work slot's block length
    (None: any).  With E_OVERRUN size is what the stream decodes to and bytes its first cap bytes; with any other error size is the count
    produced by the blocks before the failure and bytes is empty."""
    data = bytes(data)
    nbits = 8 * len(data)
    pos = 0
    out = bytearray()
    rep = {"blocks": 0, "groups": [], "max_code_length": 0, "cycle_short": False}

    def take(n):
        nonlocal pos
        if pos + n > nbits:
            raise _Fail(E_TRUNCATED)
        v = (int.from_bytes(data[pos >> 3: (pos + n + 7) >> 3], "big") >> (-(pos + n) % 8)) & ((1 << n) - 1)
        pos += n
        return v

    def fail(st):
        raise _Fail(st)

    try:
        for ch in b"BZh":
            if take(8) != ch:
                fail(E_HEADER)
        level = take(8) - 0x30
        if not 1 <= level <= 9:
            fail(E_HEADER)
        block_max = 100000 * level
        combined = 0
        while True:
            magic = take(24) << 24
            magic |= take(24)
            if magic == END_MAGIC:
                stored = take(32)
                pos = (pos + 7) // 8 * 8
                if stored != combined:
                    fail(E_CRC)
                break
            if magic != BLOCK_MAGIC:
                fail(E_MAGIC)
            block_crc = take(32)
            if take(1):
                fail(E_RANDOMISED)
            orig = take(24)
            if orig > 10 + block_max:
                fail(E_ORIGPTR)
            used16 = take(16)
            seq = []
            for i in range(16):
                if used16 >> (15 - i) & 1:
                    v = take(16)
                    seq += [16 * i + k for k in range(16) if v >> (15 - k) & 1]
            if not seq:
                fail(E_TABLE)
            alpha = len(seq) + 2
            ngroups = take(3)
            if not 2 <= ngroups <= 6:
                fail(E_TABLE)
            nsel = take(15)
            if nsel < 1:
                fail(E_TABLE)
            order = list(range(6))
            sel = []
            for i in range(nsel):
                j = 0
                while take(1):
                    j += 1
                    if j >= ngroups:
                        fail(E_TABLE)
                if i < MAX_SELECTORS:
                    order.insert(0, order.pop(j))
                    sel.append(order[0])
            tables = []
            for t in range(ngroups):
                curr = take(5)
                lens = []
                for i in range(alpha):
                    while True:
                        if not 1 <= curr <= 20:
                            fail(E_TABLE)
                        if not take(1):
                            break
                        curr += -1 if take(1) else 1
                    lens.append(curr)
                tables.append(decode_tables(lens))
                rep["max_code_length"] = max(rep["max_code_length"], max(lens))
            rep["groups"].append(ngroups)
            eob = alpha - 1
            mtf = list(seq)
            ll = bytearray()
            group_no, group_pos = -1, 0
            tab = None

            def symbol():
                nonlocal group_no, group_pos, tab
                if group_pos == 0:
                    group_no += 1
                    if group_no >= len(sel):
                        fail(E_SYMBOL)
                    group_pos = GROUP
                    tab = tables[sel[group_no]]
                group_pos -= 1
                zn, limit, base, perm = tab
                zvec = take(zn)
                while True:
                    if zn > 20:
                        fail(E_SYMBOL)
                    if zvec <= limit[zn]:
                        break
                    zn += 1
                    zvec = zvec << 1 | take(1)
                idx = zvec - base[zn]
                if not 0 <= idx < alpha:
                    fail(E_SYMBOL)
                return perm[idx]

            def room(n):
                if len(ll) + n > block_max:
                    fail(E_SYMBOL)
                if nblock_max is not None and len(ll) + n > nblock_max:
                    fail(E_WORK)

            s = symbol()
            while s != eob:
                if s <= 1:
                    es, n = -1, 1
                    while s <= 1:
                        if n >= RUN_LIMIT:
                            fail(E_SYMBOL)
                        es += n << s
                        n <<= 1
                        s = symbol()
                    es += 1
                    room(es)
                    ll += bytes([mtf[0]]) * es
                else:
                    room(1)
                    mtf.insert(0, mtf.pop(s - 1))
                    ll.append(mtf[0])
                    s = symbol()
            nblock = len(ll)
            if orig >= nblock:
                fail(E_ORIGPTR)
            col = np.frombuffer(bytes(ll), np.uint8)
            tt = np.argsort(col, kind="stable")          # tt[j] = i: the j-th byte in sorted order stands at position i
            first = np.sort(col)
            pre = bytearray(nblock)
            p = orig
            for k in range(nblock):
                pre[k] = first[p]
                p = int(tt[p])
                if p == orig and k + 1 < nblock:         # the cycle closes early: the text repeats with its period
                    rep["cycle_short"] = True
                    period = k + 1
                    for x in range(period, nblock):
                        pre[x] = pre[x - period]
                    break
            plain = unrle(pre)
            if plain is None:
                fail(E_RLE)
            out += plain
            rep["blocks"] += 1
            have = crc(plain) ^ 0xFFFFFFFF
            if have != block_crc:
                fail(E_CRC)
            combined = ((combined << 1 | combined >> 31) & 0xFFFFFFFF) ^ have
        if pos // 8 < len(data):
            fail(E_TRAILING)
        st = OK
        if cap is not None and len(out) > cap:
            st = E_OVERRUN
    except _Fail as e:
        st = e.args[0]
    used = (pos + 7) // 8
    if st == OK:
        res = (st, bytes(out), len(out), used)
    elif st == E_OVERRUN:
        res = (st, bytes(out[:cap]), len(out), used)
    else:
        res = (st, b"", len(out), used)
    return res + (rep,) if report else res
