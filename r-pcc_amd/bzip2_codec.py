"""The bzip2 back-end of basic_compressor 'bzip2' on the device (librpcc_bzip2.so).

compress() gives one bzip2 stream, as bz2.compress does: other bytes (the tables and their code lengths are the build's own, pinned to
tests/bzip2_ref.py), the same format, so bz2.decompress -- the reference's decoder -- reads it, and so does bunzip2_codec on the device.
compress_many codes a list with one copy to the device, the launches and one copy back; encode_descriptors is the device form the batch
pipeline uses, and lz4_codec.pack_containers compacts its output into .rpcc containers.  A stream the library refuses (dst_len < 0: a
length out of range) is handed to bz2.compress on the host by compress_many."""
import bz2

from . import _bzip2_lib as L
from . import entropy
from ._lib import ptr, stream

GROUP = 50


def block_limit(level=9):
    """RLE1 bytes of one block."""
    return 100000 * level - 19


def bound(n, level=9):
    """Worst-case bytes of compress() for n input bytes (rpcc_bzip2_bound): n + n / 4 bytes after RLE1 in nb blocks, 17 bits a symbol,
    6 bits a group of 50, 6450 bytes of headers, maps and tables a block, 14 bytes around them."""
    if n < 0 or n > L.MAX_INPUT or not 1 <= level <= 9:
        return 0
    m = n + n // 4
    nb = max(1, -(-m // (block_limit(level) - 4)))
    return 14 + nb * 6450 + (17 * (m + nb) + 6 * ((m + nb) // GROUP + nb) + 7) // 8


def workspace_bytes(nstreams, total_len, level=9):
    """rpcc_bzip2_workspace_bytes: the slot table, then an upper bound of the streams' work slots."""
    return (8 * nstreams + 255) // 256 * 256 + 23 * (total_len + total_len // 4) + 944 * nstreams


def encode_descriptors(addr, lens, caps, ws=None, level=9):
    """Device form of compress over descriptors: addr, lens (i64 GPU tensors [n]) the streams' device addresses and byte counts,
    caps (host ints) an upper bound of each length.  Enqueued on the current stream, nothing waited for.  -> (slots u8, dst_off i64,
    dst_len i64 GPU tensors, dst_off as numpy): stream s as a bzip2 stream at slots[dst_off[s]:][:dst_len[s]], dst_len[s] < 0 when
    its length was out of range or above its cap.  ws: the caller's work buffer of
    rpcc_bzip2_workspace_bytes(n, sum of caps, level) bytes, 16-byte aligned (allocated here when None)."""
    return entropy.encode_slots(addr, caps, lambda c: bound(c, level), lambda n, total, slots, off, cap, dst_len, w: L.check(L.lib().rpcc_bzip2_encode(
        ptr(addr), ptr(lens), n, total, level, ptr(slots), ptr(off), ptr(cap), ptr(dst_len), ptr(w), stream())),
        work_bytes=lambda n, total: L.lib().rpcc_bzip2_workspace_bytes(n, total, level), align=16, ws=ws)


def compress_many(buffers, device=None, ws=None, level=9):
    """[bytes-like or numpy array] -> [bzip2 stream bytes]: one H2D copy, the launches, one D2H copy.  A stream the library refuses is
    coded by bz2.compress on the host."""
    if not buffers:
        return []
    arrays = [entropy.as_bytes(b) for b in buffers]
    got, body, off = entropy.encode_list(arrays, device, encode_descriptors, ws=ws, level=level)
    return [body[o: o + g].tobytes() if g >= 0 else bz2.compress(a.tobytes(), level) for a, o, g in zip(arrays, off, got)]


def compress(buffer, level=9):
    """bz2.compress's form: one bzip2 stream."""
    return compress_many([buffer], level=level)[0]
