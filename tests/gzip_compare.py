"""Byte comparison of two .rpcc containers whose payloads are gzip members written by SEPARATE gzip.compress calls (basic_compressor
'gzip' / 'deflate' on the host).  gzip.compress stamps the time of the call into the four MTIME bytes of the member's header (RFC 1952:
ID1 ID2 CM FLG | MTIME, bytes 4 .. 7 | XFL OS), so two calls on either side of a second boundary differ there and nowhere else.  Everything
else stays compared: the length prefixes, the six other header bytes, every byte behind the header, and what the members decode to."""
import gzip
import struct

HEADER = 10
MTIME = slice(4, 8)


def members(blob):
    """The payloads of a container -- [int32 length | bytes] until the blob ends -- as (offset, length) pairs."""
    out, off = [], 0
    while off < len(blob):
        assert off + 4 <= len(blob), "container: a length prefix is cut off at byte %d of %d" % (off, len(blob))
        n = struct.unpack_from("i", blob, off)[0]
        assert 0 <= n <= len(blob) - off - 4, "container: payload at byte %d claims %d bytes, %d are left" % (off, n, len(blob) - off - 4)
        out.append((off + 4, n))
        off += 4 + n
    return out


def assert_equal_but_mtime(a, b, tag=None):
    """a, b: two containers of a gzip-family method, each payload one gzip member with a plain 10-byte header."""
    a, b = bytes(a), bytes(b)
    assert len(a) == len(b), (tag, "lengths", len(a), len(b))
    spans = members(a)
    assert spans == members(b), (tag, "payload spans differ")
    masked_a, masked_b = bytearray(a), bytearray(b)
    for k, (off, n) in enumerate(spans):
        for blob in (a, b):
            head = blob[off: off + HEADER]
            assert n >= HEADER + 8 and head[:3] == b"\x1f\x8b\x08" and head[3] == 0, (tag, "payload %d is no gzip member with a plain header" % k, head)
        masked_a[off + MTIME.start: off + MTIME.stop] = masked_b[off + MTIME.start: off + MTIME.stop] = b"\0\0\0\0"
    assert masked_a == masked_b, (tag, "bytes outside the MTIME fields differ")
    for k, (off, n) in enumerate(spans):
        assert gzip.decompress(a[off: off + n]) == gzip.decompress(b[off: off + n]), (tag, "payload %d decodes to other bytes" % k)
