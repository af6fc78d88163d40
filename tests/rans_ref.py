"""The 'rans' stream format, version 1, restated in plain Python: integers only, no numpy in the coding loops.
csrc_rans/rans_core.h (host build and gfx950 kernels) is held to this file byte for byte and status for status.

    header   'R' 'A' | mode u8 (0 stored, 1 coded) | width u8 (1, 2, 4) | n u32 LE | chunk_log2 u8 (8 .. 16) | 0 0 0
    stored   n bytes
    coded    width tables: m u16 LE, m x (symbol u8, freq - 1 u16 LE), symbols strictly ascending, freqs summing to 4096 (m = 0: empty plane)
             directory: ceil(n / 2^chunk_log2) payload lengths u32 LE
             payloads: min(64, k) states u32 LE in lane order, then u16 LE words

Byte i of the input is in plane i mod width; lane l of a chunk codes its bytes l, l + 64, ...  encode(..., fallback=False) gives the coded
form whatever its size (the product's encoders always apply the stored fallback): the tests use it to reach the decoders' multi-chunk
paths with 256-byte chunks, whose state flush alone is as long as the chunk."""
import struct

OK, E_CAPACITY, E_HEADER, E_TRUNCATED, E_TABLE, E_DIRECTORY, E_STATE, E_PAYLOAD = 0, -1, -2, -3, -4, -5, -6, -7
NAMES = {OK: "OK", E_CAPACITY: "E_CAPACITY", E_HEADER: "E_HEADER", E_TRUNCATED: "E_TRUNCATED", E_TABLE: "E_TABLE", E_DIRECTORY: "E_DIRECTORY",
         E_STATE: "E_STATE", E_PAYLOAD: "E_PAYLOAD"}
MAX_INPUT = 0x7E000000
HEADER = 12
PROB_BITS, PROB = 12, 4096
LOW = 1 << 16            # the encoder's start state, the decoder's end state; states live in [2^16, 2^32)
LANES = 64
DEFAULT_CHUNK_LOG2 = 15


def bound(n):
    return HEADER + n


def normalise(counts):
    """counts[256] of one plane (not all zero) -> freq[256] summing to 4096, 0 exactly where the count is 0.
    f = max(1, floor(count * 4096 / total)).  A remainder (sum < 4096) goes to the symbol with the largest f, the lowest such symbol; a
    deficit (sum > 4096: rare symbols raised to 1) is taken back one at a time, each time from the symbol with the largest f at that
    moment, the lowest such symbol."""
    total = sum(counts)
    f = [max(1, c * PROB // total) if c else 0 for c in counts]
    s = sum(f)
    if s <= PROB:
        f[f.index(max(f))] += PROB - s
        return f
    for _ in range(s - PROB):
        f[f.index(max(f))] -= 1
    return f


def _cum(f):
    cum, c = [0] * 256, 0
    for s in range(256):
        cum[s] = c
        c += f[s]
    return cum


def encode_chunk(chunk, freqs, cums, width):
    """One chunk's payload.  freqs / cums: per plane.  Rounds last to first, lanes last to first within a round, words written backwards."""
    k = len(chunk)
    lanes = min(LANES, k)
    x = [LOW] * lanes
    words = []                                   # in the order emitted: the payload holds them reversed
    for r in range((k + LANES - 1) // LANES - 1, -1, -1):
        for l in range(lanes - 1, -1, -1):
            i = r * LANES + l
            if i >= k:
                continue
            s = chunk[i]
            f, c = freqs[l % width][s], cums[l % width][s]
            if (x[l] >> 20) >= f:                # x >= f << 20
                words.append(x[l] & 0xFFFF)
                x[l] >>= 16
            x[l] = ((x[l] // f) << PROB_BITS) + x[l] % f + c
    return struct.pack("<%dI" % lanes, *x) + struct.pack("<%dH" % len(words), *reversed(words))


def header(mode, width, n, chunk_log2):
    return b"RA" + bytes([mode, width]) + struct.pack("<I", n) + bytes([chunk_log2, 0, 0, 0])


def encode(data, width=1, chunk_log2=DEFAULT_CHUNK_LOG2, fallback=True):
    data = bytes(data)
    n = len(data)
    assert width in (1, 2, 4) and 8 <= chunk_log2 <= 16 and n <= MAX_INPUT
    stored = header(0, width, n, chunk_log2) + data
    if n == 0:
        return stored
    freqs, tables = [], []
    for p in range(width):
        counts = [0] * 256
        for b in data[p::width]:
            counts[b] += 1
        f = normalise(counts) if n > p else [0] * 256
        freqs.append(f)
        present = [s for s in range(256) if f[s]]
        tables.append(struct.pack("<H", len(present)) + b"".join(struct.pack("<BH", s, f[s] - 1) for s in present))
    cums = [_cum(f) for f in freqs]
    size = 1 << chunk_log2
    payloads = [encode_chunk(data[o: o + size], freqs, cums, width) for o in range(0, n, size)]
    coded = header(1, width, n, chunk_log2) + b"".join(tables) + struct.pack("<%dI" % len(payloads), *map(len, payloads)) + b"".join(payloads)
    return coded if len(coded) < len(stored) or not fallback else stored


def parse(stream, cap):
    """The validation pass: -> (status, None) or (OK, (mode, width, n, chunk_log2, freqs per plane, [(payload offset, length)]))."""
    if len(stream) < HEADER:
        return E_TRUNCATED, None
    mode, width, chunk_log2 = stream[2], stream[3], stream[8]
    (n,) = struct.unpack_from("<I", stream, 4)
    if stream[:2] != b"RA" or mode > 1 or width not in (1, 2, 4) or not 8 <= chunk_log2 <= 16 or stream[9:12] != bytes(3) or n > MAX_INPUT:
        return E_HEADER, None
    if mode == 1 and n == 0:
        return E_HEADER, None
    if n > cap:
        return E_CAPACITY, None
    if mode == 0:
        return (OK, (0, width, n, chunk_log2, None, None)) if len(stream) == HEADER + n else (E_DIRECTORY, None)
    pos, freqs = HEADER, []
    for p in range(width):
        if pos + 2 > len(stream):
            return E_TRUNCATED, None
        (m,) = struct.unpack_from("<H", stream, pos)
        pos += 2
        if m > 256 or (m == 0) != (n <= p):
            return E_TABLE, None
        if pos + 3 * m > len(stream):
            return E_TRUNCATED, None
        f, last, total = [0] * 256, -1, 0
        for e in range(m):
            s, fm1 = struct.unpack_from("<BH", stream, pos + 3 * e)
            if s <= last or fm1 >= PROB:
                return E_TABLE, None
            f[s], last, total = fm1 + 1, s, total + fm1 + 1
        if m and total != PROB:
            return E_TABLE, None
        freqs.append(f)
        pos += 3 * m
    nch = (n + (1 << chunk_log2) - 1) >> chunk_log2
    if pos + 4 * nch > len(stream):
        return E_TRUNCATED, None
    lens = struct.unpack_from("<%dI" % nch, stream, pos)
    pos += 4 * nch
    if sum(lens) != len(stream) - pos:
        return E_DIRECTORY, None
    spans = []
    for l in lens:
        spans.append((pos, l))
        pos += l
    return OK, (1, width, n, chunk_log2, freqs, spans)


def decode_chunk(payload, k, freqs, cums, lookups, width):
    """-> (status, bytes)."""
    lanes = min(LANES, k)
    if len(payload) < 4 * lanes or (len(payload) - 4 * lanes) & 1:
        return E_PAYLOAD, b""
    x = list(struct.unpack_from("<%dI" % lanes, payload, 0))
    nw = (len(payload) - 4 * lanes) // 2
    words = struct.unpack_from("<%dH" % nw, payload, 4 * lanes)
    out, at = bytearray(k), 0
    for i in range(k):                           # byte i: round i // 64, lane i % 64 -- ascending lanes within a round
        l = i % LANES
        p = l % width
        slot = x[l] & (PROB - 1)
        s = lookups[p][slot]
        x[l] = freqs[p][s] * (x[l] >> PROB_BITS) + slot - cums[p][s]
        if x[l] < LOW:
            if at >= nw:
                return E_PAYLOAD, b""
            x[l] = (x[l] << 16) | words[at]
            at += 1
        out[i] = s
    if at != nw or any(v != LOW for v in x):
        return E_STATE, b""
    return OK, bytes(out)


def decode(stream, cap=MAX_INPUT):
    """-> (status, bytes): the bytes are empty unless the status is OK.  A stream's chunk-level status is the lowest of its chunks'."""
    stream = bytes(stream)
    st, info = parse(stream, cap)
    if st != OK:
        return st, b""
    mode, width, n, chunk_log2, freqs, spans = info
    if mode == 0:
        return OK, stream[HEADER:]
    cums = [_cum(f) for f in freqs]
    lookups = []
    for f in freqs:
        t = []
        for s in range(256):
            t += [s] * f[s]
        lookups.append(t)
    size, parts, worst = 1 << chunk_log2, [], OK
    for c, (o, l) in enumerate(spans):
        st, part = decode_chunk(stream[o: o + l], min(size, n - c * size), freqs, cums, lookups, width)
        worst = min(worst, st)
        parts.append(part)
    return (OK, b"".join(parts)) if worst == OK else (worst, b"")
