"""Reference of the build's LZ4 block encoder and a format-only LZ4 block decoder, in numpy / plain
Python.  librpcc_lz4.so must reproduce encode() byte for byte; decode_block() reads any LZ4 block.

The parse, for src[0..n):
  H(p)   = ((v(p) << 24) * 889523592379 mod 2^64) >> 50, v(p) the little-endian 40-bit value of src[p..p+5)
  c(p)   = the largest q < p with H(q) == H(p), for 0 <= p <= n-12 (every earlier position, not only inserted ones)
  accept = c(p) exists, p - c(p) <= 65535 and src[c..c+4) == src[p..p+4)
  L      = 4 + the further equal bytes src[c+4+j] == src[p+4+j], capped so that p + L <= n - 5
  greedy: i = anchor = 0; while i <= n-12: accept(i) -> emit (src[anchor..i), i-c(i), L), i += L, anchor = i; else i += 1
  then the last literals src[anchor..n) as a literal-only token."""
import struct

import numpy as np

PRIME5 = 889523592379
HASH_LOG = 14
MAX_OFFSET = 65535
MFLIMIT = 12        # a match starts at p <= n - 12
LASTLITERALS = 5    # the last 5 bytes are literals


def bound(n):
    """Worst-case size of dumps(): 4-byte header + the block."""
    return 4 + n + n // 255 + 16


def hashes(src):
    """H(p) for p = 0 .. n-5 (uint64 array)."""
    a = np.frombuffer(bytes(src), np.uint8).astype(np.uint64)
    n = a.size
    if n < 5:
        return np.zeros(0, np.uint64)
    v = np.zeros(n - 4, np.uint64)
    for k in range(5):
        v |= a[k: n - 4 + k] << np.uint64(8 * k)
    with np.errstate(over="ignore"):
        return ((v << np.uint64(24)) * np.uint64(PRIME5)) >> np.uint64(64 - HASH_LOG)


def candidates(src):
    """c(p) for p = 0 .. n-12 (int64, -1 where there is none)."""
    n = len(src)
    m = n - MFLIMIT + 1
    if m <= 0:
        return np.zeros(0, np.int64)
    h = hashes(src)[:m]
    order = np.argsort(h, kind="stable")
    hs = h[order]
    c = np.full(m, -1, np.int64)
    same = hs[1:] == hs[:-1]
    c[order[1:][same]] = order[:-1][same]
    return c


def sequences(src):
    """The greedy parse: a list of (literal start, literal length, offset, match length L), then the last literals' start."""
    src = bytes(src)
    n = len(src)
    a = np.frombuffer(src, np.uint8)
    c = candidates(src)
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
        k = 0
        while True:
            k = np.searchsorted(acc, i, side="left") if k >= acc.size or acc[k] < i else k
            if k >= acc.size:
                break
            i = int(acc[k])
            q = int(c[i])
            lim = n - LASTLITERALS - i          # L <= lim
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


def _length_bytes(v):
    out = bytearray()
    while v >= 255:
        out.append(255)
        v -= 255
    out.append(v)
    return out


def encode_block(src):
    """The raw LZ4 block of the build's parse."""
    src = bytes(src)
    seqs, last = sequences(src)
    out = bytearray()
    for lit, ll, off, L in seqs:
        ml = L - 4
        out.append((min(ll, 15) << 4) | min(ml, 15))
        if ll >= 15:
            out += _length_bytes(ll - 15)
        out += src[lit: lit + ll]
        out += struct.pack("<H", off)
        if ml >= 15:
            out += _length_bytes(ml - 15)
    ll = len(src) - last
    out.append(min(ll, 15) << 4)
    if ll >= 15:
        out += _length_bytes(ll - 15)
    out += src[last:]
    return bytes(out)


def dumps(src):
    """python-lz4 0.7.0's form: uint32 LE uncompressed size, then the block."""
    src = bytes(src)
    return struct.pack("<I", len(src)) + encode_block(src)


def decode_block(blk, n):
    """Any LZ4 block -> n bytes; ValueError on a malformed block (format only, no speed)."""
    out = bytearray()
    i = 0
    while True:
        if i >= len(blk):
            raise ValueError("truncated token")
        tok = blk[i]
        i += 1
        ll = tok >> 4
        if ll == 15:
            while True:
                if i >= len(blk):
                    raise ValueError("truncated literal length")
                b = blk[i]
                i += 1
                ll += b
                if b != 255:
                    break
        if i + ll > len(blk):
            raise ValueError("truncated literals")
        out += blk[i: i + ll]
        i += ll
        if i == len(blk):
            break
        if i + 2 > len(blk):
            raise ValueError("truncated offset")
        off = blk[i] | blk[i + 1] << 8
        i += 2
        if off == 0 or off > len(out):
            raise ValueError("bad offset %d at output %d" % (off, len(out)))
        ml = tok & 15
        if ml == 15:
            while True:
                if i >= len(blk):
                    raise ValueError("truncated match length")
                b = blk[i]
                i += 1
                ml += b
                if b != 255:
                    break
        ml += 4
        if len(out) + ml > n:
            raise ValueError("output overrun")
        s = len(out) - off
        for k in range(ml):
            out.append(out[s + k])
    if len(out) != n:
        raise ValueError("produced %d bytes, header says %d" % (len(out), n))
    return bytes(out)


def loads(blob):
    blob = bytes(blob)
    if len(blob) < 4:
        raise ValueError("truncated header")
    (n,) = struct.unpack_from("<I", blob)
    if n == 0 and len(blob) == 4:
        return b""
    return decode_block(blob[4:], n)
