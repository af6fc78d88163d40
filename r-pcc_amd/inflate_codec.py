"""The gzip decoder of basic_compressor 'deflate' / 'gzip' on the device (librpcc_inflate.so).

decompress() reads one gzip member as gzip.decompress does -- whoever wrote it: deflate_codec, gzip.compress or any other deflate
encoder -- and returns the same bytes; what gzip.decompress refuses is refused (ValueError), and so is a second member, which
gzip.decompress would concatenate.  decode_many decodes a list with one copy to the device, one launch and one copy back;
decode_descriptors is the device form: each stream lands at an offset of the caller's choice."""
import struct

import numpy as np
import torch

from . import _inflate_lib as L
from . import entropy
from ._lib import ptr, stream

MAX_RATIO = 1032      # deflate's largest expansion: 258 bytes from a 2-bit match

_STATUS = {L.E_TRUNCATED: "the stream ends early (header, bits, stored bytes or trailer)", L.E_HEADER: "not a gzip member (magic or method)",
           L.E_BTYPE: "block type 3", L.E_STORED: "stored block: LEN and NLEN disagree", L.E_TABLE: "invalid code lengths",
           L.E_SYMBOL: "invalid code or symbol", L.E_OFFSET: "distance before the start of the output",
           L.E_OVERRUN: "more output than the member's size field says", L.E_CRC: "CRC-32 mismatch", L.E_SIZE: "size field mismatch",
           L.E_TRAILING: "data after the member (a second member, or bytes other than zero)"}


def status_text(st):
    return _STATUS.get(int(st), "error")


def decode_descriptors(addr, lens, dst, dst_off, dst_cap):
    """Device form: stream s reads lens[s] bytes at the device address addr[s] and is written at dst[dst_off[s]:], at most dst_cap[s]
    bytes (addr, lens, dst_off, dst_cap: i64 GPU tensors [n]; dst: u8 GPU tensor).  Enqueued on the current stream, nothing waited
    for.  -> (dst_len i64 [n], status i32 [n]) GPU tensors."""
    n = addr.numel()
    dst_len = torch.empty(n, dtype=torch.int64, device=addr.device)
    status = torch.empty(n, dtype=torch.int32, device=addr.device)
    if n:
        L.check(L.lib().rpcc_inflate_decode(ptr(addr), ptr(lens), n, ptr(dst), ptr(dst_off), ptr(dst_cap), ptr(dst_len), ptr(status), stream()))
    return dst_len, status


def size_fields(a):
    """(the size the member states if nothing follows it, the largest size it can state if zero bytes follow it), each capped at what
    deflate can produce from that many bytes.  ISIZE is the trailer's last field and its own high bytes are usually zero, so where a
    member ends among trailing zero bytes cannot be told without decoding it: a member with a size other than 0 ends 0 to 3 bytes behind
    its last byte that is not zero."""
    if a.size < 18:
        return 0, 0
    end = a.size
    while end > 18 and a[end - 1] == 0:
        end -= 1
    top = MAX_RATIO * a.size
    alone = struct.unpack_from("<I", a, a.size - 4)[0]
    padded = max(struct.unpack_from("<I", a, e - 4)[0] for e in range(end, min(end + 3, a.size) + 1))
    return min(alone, top), min(max(alone, padded), top)


def _decode(n, m, out, cols, status, work):
    L.check(L.lib().rpcc_inflate_decode(ptr(m[0]), ptr(m[1]), n, ptr(out), ptr(m[2]), ptr(m[3]), ptr(cols[0]), ptr(status), stream()))


def decode_many(blobs, device=None):
    """[gzip member bytes] -> (status int32 [n]: 0 or RPCC_INFLATE_E_*, [bytes, None where the status is not 0]): one H2D copy, one
    launch, one D2H copy.  Each slot is sized on the host from the member's size field, so a member that states a wrong size ends in
    E_OVERRUN or E_SIZE.  (Members that fail and are followed by zero bytes go through a second launch with the largest size their
    last bytes can mean, see size_fields: padding is not something this project writes.)"""
    if not blobs:
        return np.zeros(0, np.int32), []
    dev = entropy.device_of(device)
    arrays = [entropy.as_bytes(b) for b in blobs]
    sizes = np.array([size_fields(a) for a in arrays], np.int64).reshape(-1, 2)
    res = entropy.decode_list(arrays, sizes[:, 0], dev, _decode)
    st, outs = res[0], entropy.slot_bytes(*res)
    again = np.flatnonzero((st != L.OK) & (sizes[:, 1] > sizes[:, 0]))
    if again.size:
        res = entropy.decode_list([arrays[k] for k in again], sizes[again, 1], dev, _decode)
        for k, s, o in zip(again, res[0], entropy.slot_bytes(*res)):
            st[k], outs[k] = s, o
    return st, outs


def decompress_many(blobs, device=None):
    """[gzip member bytes] -> [bytes].  ValueError names the first bad stream."""
    st, outs = decode_many(blobs, device)
    entropy.raise_first_bad(st, "gzip", _STATUS)
    return outs


def decompress(blob):
    """gzip.decompress for one member; ValueError on a bad stream."""
    return decompress_many([blob])[0]
