"""Reference of the build's deflate encoder in numpy / plain Python.  librpcc_deflate.so must reproduce
compress() byte for byte; every stream is a gzip member that gzip.decompress reads.

  parse    section 11's greedy parse (lz4_ref.candidates: hash5 at hashLog 14 over every earlier position, 4 equal bytes, no
           backward extension, p <= n-12, p + L <= n-5) with a maximum offset of 32768
  split    a match longer than 258 leaves in chunks of 258, the last two so that neither is shorter than 3
  codes    two-queue Huffman over (f, symbol)-sorted leaves, limited to 15 bits (7 for the code-length code) by moving leaves
           down from the deepest level that has one, canonical codes
  block    one dynamic block per stream, or stored blocks where that is not larger"""
import struct
import zlib

import numpy as np

import lz4_ref

MAX_OFFSET = 32768
MFLIMIT = lz4_ref.MFLIMIT
LASTLITERALS = lz4_ref.LASTLITERALS
MAX_MATCH = 258
MIN_MATCH = 3
HEADER = bytes([0x1F, 0x8B, 8, 0, 0, 0, 0, 0, 0, 0xFF])
STORED_MAX = 65535

LEN_BASE = np.array([3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258])
LEN_EXTRA = np.array([0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0])
DIST_BASE = np.array([1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
                      8193, 12289, 16385, 24577])
DIST_EXTRA = np.array([0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13])
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


def stored_blocks(n):
    return max(1, -(-n // STORED_MAX))


def bound(n):
    """Worst-case size of compress(): header, trailer and stored blocks."""
    return 18 + n + 5 * stored_blocks(n)


def sequences(src):
    """lz4_ref.sequences with the deflate window: (literal start, literal length, offset, L) per match, then the last literals' start."""
    src = bytes(src)
    n = len(src)
    a = np.frombuffer(src, np.uint8)
    c = lz4_ref.candidates(src)
    m = c.size
    seqs = []
    anchor = 0
    if m:
        p = np.arange(m)
        ok = (c >= 0) & (p - c <= MAX_OFFSET)
        cc = np.where(ok, c, 0)
        for k in range(4):
            ok &= a[cc + k] == a[p + k]
        acc = np.flatnonzero(ok)
        i = 0
        while True:
            k = np.searchsorted(acc, i, side="left")
            if k >= acc.size:
                break
            i = int(acc[k])
            q = int(c[i])
            lim = n - LASTLITERALS - i
            L = 4
            while L < lim:
                step = min(4096, lim - L)
                neq = np.flatnonzero(a[q + L: q + L + step] != a[i + L: i + L + step])
                if neq.size:
                    L += int(neq[0])
                    break
                L += step
            seqs.append((anchor, i - anchor, i - q, L))
            i += L
            anchor = i
    return seqs, anchor


def split(L):
    """The deflate match lengths of one match of length L >= 3."""
    out = []
    while L > MAX_MATCH:
        t = MAX_MATCH if L - MAX_MATCH >= MIN_MATCH else L - MIN_MATCH
        out.append(t)
        L -= t
    out.append(L)
    return out


def symbols(src):
    """-> (kind, a, b) arrays, one entry per deflate symbol before end-of-block: kind 0 a literal a, kind 1 a match of length a at distance b."""
    src = bytes(src)
    a = np.frombuffer(src, np.uint8)
    seqs, last = sequences(src)
    kind, va, vb = [], [], []
    for lit, ll, off, L in seqs:
        if ll:
            kind.append(np.zeros(ll, np.int64))
            va.append(a[lit: lit + ll].astype(np.int64))
            vb.append(np.zeros(ll, np.int64))
        ch = split(L)
        kind.append(np.ones(len(ch), np.int64))
        va.append(np.array(ch, np.int64))
        vb.append(np.full(len(ch), off, np.int64))
    ll = len(src) - last
    kind.append(np.zeros(ll, np.int64))
    va.append(a[last:].astype(np.int64))
    vb.append(np.zeros(ll, np.int64))
    return np.concatenate(kind), np.concatenate(va), np.concatenate(vb)


def code_lengths(freq, maxbits):
    """The code lengths of an alphabet with frequencies freq (a list; fewer than two used symbols are filled up from symbol 0)."""
    f = [int(x) for x in freq]
    while sum(1 for x in f if x > 0) < 2:
        f[f.index(0)] = 1
    order = sorted((x, s) for s, x in enumerate(f) if x > 0)
    n = len(order)
    # nodes 0 .. n-1 are the leaves in sorted order, n .. 2n-2 the internal nodes in creation order
    weight = [x for x, _ in order] + [0] * (n - 1)
    parent = [0] * (2 * n - 1)
    li, ii = 0, n
    for new in range(n, 2 * n - 1):
        for _ in range(2):
            if li < n and (ii >= new or weight[li] <= weight[ii]):
                pick = li
                li += 1
            else:
                pick = ii
                ii += 1
            weight[new] += weight[pick]
            parent[pick] = new
    depth = [0] * (2 * n - 1)
    for k in range(2 * n - 3, -1, -1):
        depth[k] = depth[parent[k]] + 1
    num = [0] * (maxbits + 1)
    for k in range(n):
        num[min(depth[k], maxbits)] += 1
    total = sum(num[i] << (maxbits - i) for i in range(1, maxbits + 1))
    while total != 1 << maxbits:
        num[maxbits] -= 1
        i = max(j for j in range(1, maxbits) if num[j] > 0)
        num[i] -= 1
        num[i + 1] += 2
        total -= 1
    lens = [0] * len(f)
    k = n
    for i in range(1, maxbits + 1):
        for _ in range(num[i]):
            k -= 1
            lens[order[k][1]] = i
    return lens


def canonical_codes(lens):
    """RFC 1951 3.2.2 codes of the lengths, bit-reversed for the LSB-first stream."""
    maxbits = max(lens)
    count = [0] * (maxbits + 2)
    for x in lens:
        if x:
            count[x] += 1
    nxt = [0] * (maxbits + 2)
    code = 0
    for b in range(1, maxbits + 1):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = [0] * len(lens)
    for s, x in enumerate(lens):
        if x:
            c = nxt[x]
            nxt[x] += 1
            out[s] = int(format(c, "0%db" % x)[::-1], 2)
    return out


def run_length(seq):
    """The code-length symbols of the sequence: a list of (symbol, extra value, extra bits)."""
    out = []
    i, n = 0, len(seq)
    while i < n:
        v = seq[i]
        r = 1
        while i + r < n and seq[i + r] == v:
            r += 1
        if v == 0:
            if r >= 11:
                t = min(r, 138)
                out.append((18, t - 11, 7))
            elif r >= 3:
                t = r
                out.append((17, t - 3, 3))
            else:
                t = 1
                out.append((0, 0, 0))
            i += t
        else:
            out.append((v, 0, 0))
            rest = r - 1
            while rest >= 3:
                t = min(rest, 6)
                out.append((16, t - 3, 2))
                rest -= t
            out += [(v, 0, 0)] * rest
            i += r
    return out


def _pack(vals, bits):
    """Values of bits[k] bits each, LSB first, back to back -> (bytes, total bits)."""
    vals, bits = np.asarray(vals, np.int64), np.asarray(bits, np.int64)
    off = np.cumsum(bits) - bits
    total = int(bits.sum())
    out = np.zeros((total + 7) // 8 * 8, np.uint8)
    for k in range(int(bits.max()) if bits.size else 0):
        sel = bits > k
        out[off[sel] + k] = (vals[sel] >> k) & 1
    return np.packbits(out, bitorder="little").tobytes(), total


def tables(src):
    """-> dict with the symbols, the three codes' lengths and the header's fields of the dynamic block of src."""
    kind, va, vb = symbols(src)
    lit = kind == 0
    lsym = np.searchsorted(LEN_BASE, va[~lit], side="right") - 1
    dsym = np.searchsorted(DIST_BASE, vb[~lit], side="right") - 1
    fl = np.bincount(va[lit], minlength=286) + np.bincount(257 + lsym, minlength=286)
    fl[256] = 1
    fd = np.bincount(dsym, minlength=30)
    ll = code_lengths(fl.tolist(), 15)
    dl = code_lengths(fd.tolist(), 15)
    hlit = max(257, max(s for s in range(286) if ll[s]) + 1)
    hdist = max(s for s in range(30) if dl[s]) + 1
    rl = run_length(ll[:hlit] + dl[:hdist])
    fc = np.bincount([s for s, _, _ in rl], minlength=19)
    cl = code_lengths(fc.tolist(), 7)
    hclen = max(4, max(k for k in range(19) if cl[CL_ORDER[k]]) + 1)
    return dict(kind=kind, va=va, vb=vb, lsym=lsym, dsym=dsym, ll=ll, dl=dl, cl=cl, hlit=hlit, hdist=hdist, hclen=hclen, rl=rl)


def dynamic_block(src):
    """The one final dynamic block of src -> (bytes, bits)."""
    t = tables(src)
    lc, dc, cc = canonical_codes(t["ll"]), canonical_codes(t["dl"]), canonical_codes(t["cl"])
    vals = [1, 2, t["hlit"] - 257, t["hdist"] - 1, t["hclen"] - 4]
    bits = [1, 2, 5, 5, 4]
    for k in range(t["hclen"]):
        vals.append(t["cl"][CL_ORDER[k]])
        bits.append(3)
    for s, ev, eb in t["rl"]:
        vals += [cc[s], ev]
        bits += [t["cl"][s], eb]
    kind, va, vb = t["kind"], t["va"], t["vb"]
    n = kind.size
    ll, dl, lc, dc = np.array(t["ll"]), np.array(t["dl"]), np.array(lc), np.array(dc)
    # four fields per symbol: code, length extra, distance code, distance extra (0 bits where absent)
    v4 = np.zeros((n, 4), np.int64)
    b4 = np.zeros((n, 4), np.int64)
    lit = kind == 0
    v4[lit, 0], b4[lit, 0] = lc[va[lit]], ll[va[lit]]
    ls, ds = t["lsym"], t["dsym"]
    v4[~lit, 0], b4[~lit, 0] = lc[257 + ls], ll[257 + ls]
    v4[~lit, 1], b4[~lit, 1] = va[~lit] - LEN_BASE[ls], LEN_EXTRA[ls]
    v4[~lit, 2], b4[~lit, 2] = dc[ds], dl[ds]
    v4[~lit, 3], b4[~lit, 3] = vb[~lit] - DIST_BASE[ds], DIST_EXTRA[ds]
    vals = np.concatenate([np.array(vals, np.int64), v4.reshape(-1), [lc[256]]])
    bits = np.concatenate([np.array(bits, np.int64), b4.reshape(-1), [ll[256]]])
    return _pack(vals, bits)


def stored(src):
    src = bytes(src)
    out = bytearray()
    nb = stored_blocks(len(src))
    for k in range(nb):
        part = src[k * STORED_MAX: (k + 1) * STORED_MAX]
        out += struct.pack("<BHH", 1 if k == nb - 1 else 0, len(part), len(part) ^ 0xFFFF) + part
    return bytes(out)


def body(src):
    """The raw deflate stream of src."""
    src = bytes(src)
    n = len(src)
    blk, bits = dynamic_block(src)
    if (bits + 7) // 8 <= n + 5 * stored_blocks(n):
        return blk
    return stored(src)


def compress(src):
    """The gzip member of src."""
    src = bytes(src)
    return HEADER + body(src) + struct.pack("<II", zlib.crc32(src), len(src) & 0xFFFFFFFF)
