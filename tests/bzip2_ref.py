"""The bzip2 encoder of librpcc_bzip2.so stated in Python: compress(data, level) gives the bytes the kernels give.

The stream is valid bzip2 -- bz2.decompress reads it -- but not libbz2's: RLE1, the rotation sort and MTF / RLE2 are the format's, the
block cut, the number of tables, their initial lengths, the four refinement passes and the length-limited code lengths are the build's
own rules, each stated once below.  stats(data, level) gives what the cases are chosen by (nMTF, groups, tables, Kraft repairs)."""
import zlib

import numpy as np

GROUP = 50
MAX_LEN = 17
PASSES = 4
_REV8 = bytes(int("{:08b}".format(i)[::-1], 2) for i in range(256))


def block_limit(level):
    """RLE1 bytes of one block."""
    return 100000 * level - 19


def crc(data):
    """bzip2's CRC (0x04C11DB7, MSB first, initial and final complement): zlib's, with every byte and the result bit-reversed."""
    v = zlib.crc32(bytes(data).translate(_REV8)) & 0xFFFFFFFF
    return int("{:032b}".format(v)[::-1], 2)


def sub_runs(data):
    """The maximal runs of equal bytes, cut at 255 -> (start, length) int64 arrays."""
    a = np.frombuffer(bytes(data), np.uint8)
    heads = np.flatnonzero(np.concatenate(([True], a[1:] != a[:-1])))
    lens = np.diff(np.concatenate((heads, [a.size])))
    k = (lens + 254) // 255
    first = np.repeat(np.cumsum(k) - k, k)
    j = np.arange(int(k.sum())) - first
    start = np.repeat(heads, k) + 255 * j
    return start, np.minimum(np.repeat(lens, k) - 255 * j, 255)


def rle1_size(n):
    """The most RLE1 bytes n input bytes give: five for every four."""
    return n + n // 4


def blocks(data, level):
    """-> [(raw bytes of the block, its RLE1 bytes)]: the longest prefix of whole sub-runs within block_limit(level)."""
    a = np.frombuffer(bytes(data), np.uint8)
    if not a.size:
        return []
    start, ln = sub_runs(data)
    size = np.minimum(ln, 4) + (ln >= 4)
    end = np.cumsum(size)
    out, r0, base = [], 0, 0
    while r0 < ln.size:
        r1 = int(np.searchsorted(end, base + block_limit(level), side="right"))
        lo, hi = int(start[r0]), int(start[r1 - 1] + ln[r1 - 1])
        s, l, z = start[r0:r1], ln[r0:r1], size[r0:r1]
        o = np.cumsum(z) - z
        rle = np.repeat(a[s], z)
        rle[(o + 4)[l >= 4]] = (l - 4)[l >= 4]
        out.append((a[lo:hi].tobytes(), rle))
        base, r0 = int(end[r1 - 1]), r1
    return out


def rotation_sort(b):
    """The rotations of b in ascending order, equal ones by ascending start -> (sa, doubling rounds, the last h)."""
    n = b.size
    idx = np.arange(n)
    sa = np.argsort(b, kind="stable")
    key = b[sa].astype(np.int64)
    rank = np.empty(n, np.int64)
    rank[sa] = np.maximum.accumulate(np.where(np.concatenate(([True], key[1:] != key[:-1])), idx, 0))
    h, rounds = 1, 0
    while h < n and np.unique(rank).size < n:
        key = rank * n + rank[(idx + h) % n]
        sa = np.argsort(key, kind="stable")
        k = key[sa]
        rank = np.empty(n, np.int64)
        rank[sa] = np.maximum.accumulate(np.where(np.concatenate(([True], k[1:] != k[:-1])), idx, 0))
        h *= 2
        rounds += 1
    return np.argsort(rank, kind="stable"), rounds, h


def mtf_rle2(last, used, zruns=None):
    """Move-to-front over the used byte values, zero runs as RUNA / RUNB (bijective base 2, low digit first) -> symbols with EOB.
    zruns (a list): receives the zero runs' lengths, the last one being the run at the block's end (0: none)."""
    order = list(used)
    out, run = [], 0

    def flush():
        nonlocal run
        if zruns is not None:
            zruns.append(run)
        while run > 0:
            out.append(0 if run & 1 else 1)      # RUNA = digit 1, RUNB = digit 2
            run = (run - 1) >> 1
    for v in last.tolist():
        p = order.index(v)
        if p == 0:
            run += 1
            continue
        flush()
        out.append(p + 1)
        order.insert(0, order.pop(p))
    flush()
    out.append(len(used) + 1)
    return np.array(out, np.int64)


def code_lengths(count, maxbits=MAX_LEN, repairs=None):
    """huffman_code of csrc_deflate/deflate_kernels.hip over counts that are all positive: symbols ordered by (count, symbol), a
    two-queue merge with the leaf first on a tie, depths clamped to maxbits, the Kraft sum repaired one leaf at a time, the longest
    lengths to the least frequent symbols."""
    n = len(count)
    order = sorted(range(n), key=lambda s: (count[s], s))
    weight = [count[s] for s in order] + [0] * (n - 1)
    parent = [0] * (2 * n - 1)
    li, ii = 0, n
    for nw in range(n, 2 * n - 1):
        w = 0
        for _ in range(2):
            if li < n and (ii >= nw or weight[li] <= weight[ii]):
                pick, li = li, li + 1
            else:
                pick, ii = ii, ii + 1
            w += weight[pick]
            parent[pick] = nw
        weight[nw] = w
    depth = [0] * (2 * n - 1)
    for k in range(2 * n - 3, -1, -1):
        depth[k] = depth[parent[k]] + 1
    num = [0] * (maxbits + 1)
    for k in range(n):
        num[min(depth[k], maxbits)] += 1
    total = sum(num[i] << (maxbits - i) for i in range(1, maxbits + 1))
    while total != 1 << maxbits:
        num[maxbits] -= 1
        i = maxbits - 1
        while num[i] == 0:
            i -= 1
        num[i] -= 1
        num[i + 1] += 2
        total -= 1
        if repairs is not None:
            repairs[0] += 1
    lens = [0] * n
    k = n
    for i in range(1, maxbits + 1):
        for _ in range(num[i]):
            k -= 1
            lens[order[k]] = i
    return lens


def table_count(nmtf):
    return 2 if nmtf < 200 else 3 if nmtf < 600 else 4 if nmtf < 1200 else 5 if nmtf < 2400 else 6


def initial_lengths(freq, nmtf, nt):
    alpha = len(freq)
    lens = np.full((nt, alpha), 15, np.int64)
    rem, gs = nmtf, 0
    for t in range(nt, 0, -1):
        tf, ge, af = rem // t, gs - 1, 0
        while af < tf and ge < alpha - 1:
            ge += 1
            af += int(freq[ge])
        if ge > gs and t != nt and t != 1 and (nt - t) % 2 == 1:
            af -= int(freq[ge])
            ge -= 1
        lens[t - 1, gs: ge + 1] = 0
        gs, rem = ge + 1, rem - af
    return lens


def tables(sym, alpha, repairs=None):
    """-> (lengths [nt, alpha], selectors [groups])."""
    nmtf = sym.size
    nt = table_count(nmtf)
    ng = (nmtf + GROUP - 1) // GROUP
    lens = initial_lengths(np.bincount(sym, minlength=alpha), nmtf, nt)
    pad = np.zeros(ng * GROUP, np.int64)
    pad[:nmtf] = sym
    live = (np.arange(ng * GROUP) < nmtf).reshape(ng, GROUP)
    sel = None
    for _ in range(PASSES):
        cost = (lens[:, pad].reshape(nt, ng, GROUP) * live).sum(2)
        sel = np.argmin(cost, 0)                 # ties: the lowest index
        tab = np.repeat(sel, GROUP)[:nmtf]
        for t in range(nt):
            cnt = np.maximum(np.bincount(sym[tab == t], minlength=alpha), 1)
            lens[t] = code_lengths(cnt.tolist(), MAX_LEN, repairs)
    return lens, sel


def canonical(lens):
    """Codes MSB first, ascending symbol within a length."""
    code, c = np.zeros(len(lens), np.int64), 0
    for b in range(1, MAX_LEN + 1):
        for s in np.flatnonzero(np.asarray(lens) == b):
            code[s] = c
            c += 1
        c <<= 1
    return code


class Bits:
    def __init__(self):
        self.v, self.n = [], []

    def put(self, v, n):
        self.v.append(np.atleast_1d(np.asarray(v, np.int64)))
        self.n.append(np.atleast_1d(np.asarray(n, np.int64)))

    def bytes(self):
        v, n = np.concatenate(self.v), np.concatenate(self.n)
        start = np.cumsum(n) - n
        bits = np.zeros(int(n.sum()) + 7, np.uint8)
        for b in range(int(n.max())):
            m = n > b
            bits[start[m] + b] = (v[m] >> (n[m] - 1 - b)) & 1
        return np.packbits(bits[: (int(n.sum()) + 7) // 8 * 8]).tobytes()


def encode_block(w, raw, rle, info=None):
    n = rle.size
    sa, rounds, h = rotation_sort(rle)
    orig = int(np.flatnonzero(sa == 0)[0])
    last = rle[(sa - 1) % n]
    used = np.flatnonzero(np.bincount(rle, minlength=256))
    zruns = []
    sym = mtf_rle2(last, used.tolist(), zruns)
    alpha = used.size + 2
    repairs = [0]
    lens, sel = tables(sym, alpha, repairs)
    nt = lens.shape[0]
    if info is not None:
        info.append(dict(nblock=n, nmtf=int(sym.size), groups=int(sel.size), tables=nt, repairs=repairs[0], rounds=rounds, h=h, alpha=alpha,
                         zruns=zruns))
    w.put([0x314159, 0x265359, crc(raw)], [24, 24, 32])
    w.put([0, orig], [1, 24])
    inuse = np.zeros(256, np.int64)
    inuse[used] = 1
    rows = inuse.reshape(16, 16)
    w.put(int("".join(str(int(r.any())) for r in rows), 2), 16)
    for r in rows:
        if r.any():
            w.put(int("".join(map(str, r)), 2), 16)
    w.put([nt, sel.size], [3, 15])
    order = list(range(nt))
    for s in sel.tolist():
        j = order.index(s)
        w.put((1 << (j + 1)) - 2, j + 1)         # j ones, a zero
        order.insert(0, order.pop(j))
    for t in range(nt):
        cur = int(lens[t, 0])
        w.put(cur, 5)
        for L in lens[t].tolist():
            while cur < L:
                w.put(2, 2)
                cur += 1
            while cur > L:
                w.put(3, 2)
                cur -= 1
            w.put(0, 1)
    codes = np.stack([canonical(lens[t]) for t in range(nt)])
    tab = np.repeat(sel, GROUP)[: sym.size]
    w.put(codes[tab, sym], lens[tab, sym])
    return crc(raw)


def compress(data, level=9, info=None):
    assert 1 <= level <= 9
    w = Bits()
    w.put([0x42, 0x5A, 0x68, 0x30 + level], [8, 8, 8, 8])
    combined = 0
    for raw, rle in blocks(data, level):
        c = encode_block(w, raw, rle, info)
        combined = ((combined << 1 | combined >> 31) & 0xFFFFFFFF) ^ c
    w.put([0x177245, 0x385090, combined], [24, 24, 32])
    return w.bytes()


def stats(data, level=9):
    info = []
    compress(data, level, info)
    return info


def bound(n, level=9):
    """rpcc_bzip2_bound: the worst case of the rules above.  m = rle1_size(n) block bytes in all; a block of b bytes gives at most
    b + 1 symbols of MAX_LEN bits, (b + 1) / 50 + 1 selectors of 6 bits, 6 tables of 5 + 258 * (2 * 16 + 1) bits... stated in bytes:
    header 4, end 10, per block 19 (magics, CRC, origin, maps' first word) + 32 (maps) + 3 (tables, selectors' counts) + 6 * 1066
    (tables), and 17 bits a symbol, 6 bits a group."""
    if n < 0 or n > MAX_INPUT:
        return 0
    m = rle1_size(n)
    nb = max(1, -(-m // (block_limit(level) - 4)))      # a block is cut at most 4 bytes below the limit (a sub-run gives at most 5)
    sym_bits = 17 * (m + nb)
    sel_bits = 6 * ((m + nb) // GROUP + nb)
    return 14 + nb * (19 + 32 + 3 + 6 * 1066) + (sym_bits + sel_bits + 7) // 8


MAX_INPUT = 0x7E000000


def block_cap(n, level=9):
    """The RLE1 bytes the work slot of a stream of n bytes holds (bze_block_cap)."""
    return min(rle1_size(n), block_limit(level))


def work_bytes(m):
    """bze_layout(m).bytes: four uint32 and two bytes per block byte (16-aligned, 16 at least), the symbols, the selectors, and a
    recency list and a start list of 256 bytes for every 256 block bytes."""
    m16 = max(16, (m + 15) // 16 * 16)
    chunks = m16 // 256 + 1
    return 18 * m16 + 2 * m16 + 32 + (m16 // GROUP + 2 + 15) // 16 * 16 + 512 * chunks


def workspace_bytes(nstreams, total_len):
    """rpcc_bzip2_workspace_bytes: the slot table, then an upper bound of the slots (work_bytes(m) <= 23 m16 + 576, m16 <= n + n / 4 + 16)."""
    return (8 * nstreams + 255) // 256 * 256 + 23 * rle1_size(total_len) + 944 * nstreams
