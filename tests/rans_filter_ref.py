"""The 'rans' stream format, version 2 ("Version 2: the delta filter"), restated in plain Python on top of
tests/rans_ref.py, which stays the statement of version 1 and of the coder.  Version 2 adds one stream form:

    header   'R' 'B' | mode u8 = 1 | width u8 (1, 2, 4) | n u32 LE (> 0) | chunk_log2 u8 (8 .. 16) | filter u8 = 1 | 0 0
    then     tables, directory and payloads exactly as in a coded version-1 stream, over the FILTERED bytes

Filter 1 (delta + zigzag) works on the E = n // width whole elements u[e] (width bytes, little-endian, unsigned); the n % width bytes
behind them pass through.  With C = 2^chunk_log2 / width elements to a chunk: prev = 0 where e % C == 0, else u[e - 1];
d = (u[e] - prev) mod 2^(8 width); z = ((d << 1) ^ (d >>arithmetic (8 width - 1))) mod 2^(8 width); the coder sees the bytes of z,
byte i still in plane i mod width.  Inverse: d = (z >> 1) ^ -(z & 1), u[e] = prev + d, all modulo 2^(8 width).

There is no stored form under 'RB': an encoder whose filtered coded stream is not smaller than 12 + n writes the version-1 stored
stream.  parse / decode read both magics; every status and the order of the checks are version 1's."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rans_ref as R  # noqa: E402

FILTER_NONE, FILTER_DELTA = 0, 1
OK, HEADER, DEFAULT_CHUNK_LOG2, MAX_INPUT, NAMES = R.OK, R.HEADER, R.DEFAULT_CHUNK_LOG2, R.MAX_INPUT, R.NAMES


def forward(data, width, chunk_log2):
    """The bytes the coder sees."""
    data = bytes(data)
    bits, per = 8 * width, (1 << chunk_log2) // width
    mask = (1 << bits) - 1
    out, prev = bytearray(data), 0
    for e in range(len(data) // width):
        u = int.from_bytes(data[e * width: (e + 1) * width], "little")
        d = (u - (0 if e % per == 0 else prev)) & mask
        z = ((d << 1) ^ (mask if d >> (bits - 1) else 0)) & mask
        out[e * width: (e + 1) * width] = z.to_bytes(width, "little")
        prev = u
    return bytes(out)


def inverse(data, width, chunk_log2):
    """The bytes forward() was given."""
    data = bytes(data)
    bits, per = 8 * width, (1 << chunk_log2) // width
    mask = (1 << bits) - 1
    out, prev = bytearray(data), 0
    for e in range(len(data) // width):
        z = int.from_bytes(data[e * width: (e + 1) * width], "little")
        d = (z >> 1) ^ (mask if z & 1 else 0)
        prev = ((0 if e % per == 0 else prev) + d) & mask
        out[e * width: (e + 1) * width] = prev.to_bytes(width, "little")
    return bytes(out)


def header(width, n, chunk_log2):
    """The version-2 header (mode 1, filter 1)."""
    return b"RB" + bytes([1, width]) + R.header(1, width, n, chunk_log2)[4:9] + bytes([FILTER_DELTA, 0, 0])


def encode(data, width=1, chunk_log2=DEFAULT_CHUNK_LOG2, filter=FILTER_NONE, fallback=True):
    """filter 0: rans_ref.encode's bytes.  filter 1: the 'RB' stream, or (fallback) the version-1 stored stream when that is not larger;
    no bytes have no coded form, so they are the stored stream whatever fallback says."""
    assert filter in (FILTER_NONE, FILTER_DELTA)
    data = bytes(data)
    if filter == FILTER_NONE:
        return R.encode(data, width, chunk_log2, fallback=fallback)
    stored = R.header(0, width, len(data), chunk_log2) + data
    if not data:
        return stored
    coded = R.encode(forward(data, width, chunk_log2), width, chunk_log2, fallback=False)
    coded = header(width, len(data), chunk_log2) + coded[HEADER:]
    return coded if len(coded) < len(stored) or not fallback else stored


def _as_version1(stream):
    """An 'RB' stream whose own header rules hold -> the version-1 stream of its filtered bytes; else None."""
    if stream[2] != 1 or stream[9] != FILTER_DELTA or stream[10:12] != bytes(2):
        return None
    return b"RA" + stream[2:9] + bytes(3) + stream[HEADER:]


def parse(stream, cap):
    """rans_ref.parse for both magics: -> (status, None) or (OK, (mode, width, n, chunk_log2, freqs, spans, filter))."""
    stream = bytes(stream)
    filt = FILTER_NONE
    if len(stream) >= HEADER and stream[:2] == b"RB":
        stream, filt = _as_version1(stream), FILTER_DELTA
        if stream is None:
            return R.E_HEADER, None
    st, info = R.parse(stream, cap)
    return (st, info + (filt,)) if st == OK else (st, None)


def decode(stream, cap=MAX_INPUT):
    """-> (status, bytes), as rans_ref.decode, for both magics."""
    stream = bytes(stream)
    if len(stream) < HEADER or stream[:2] != b"RB":
        return R.decode(stream, cap)
    v1 = _as_version1(stream)
    if v1 is None:
        return R.E_HEADER, b""
    st, out = R.decode(v1, cap)
    return (st, inverse(out, stream[3], stream[8])) if st == OK else (st, b"")
