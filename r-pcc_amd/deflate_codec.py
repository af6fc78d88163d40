"""The gzip back-end of basic_compressor 'deflate' / 'gzip' on the device (librpcc_deflate.so).

compress() gives one gzip member, as gzip.compress does: other bytes (the parse and the code lengths are the build's own), the
same format, so gzip.decompress -- the reference's decoder -- reads it, and so does inflate_codec on the device.  compress_many codes a
list with one copy to the device, the launches and one copy back; encode_descriptors is the device form the batch pipeline
uses, and lz4_codec.pack_containers compacts its output into .rpcc containers."""
from . import _deflate_lib as L
from . import entropy
from ._lib import ptr, stream


def bound(n):
    """Worst-case bytes of compress() for n input bytes: header, trailer and stored blocks of at most 65535 bytes."""
    return 18 + n + 5 * max(1, -(-n // 65535))


def encode_descriptors(addr, lens, caps, ws=None):
    """Device form of compress over descriptors: addr, lens (i64 GPU tensors [n]) the streams' device addresses and byte counts,
    caps (host ints) an upper bound of each length.  Enqueued on the current stream, nothing waited for.  -> (slots u8, dst_off i64,
    dst_len i64 GPU tensors, dst_off as numpy): stream s as a gzip member at slots[dst_off[s]:][:dst_len[s]], dst_len[s] < 0 when
    its length was out of range or above its cap.  ws: the caller's work buffer of rpcc_deflate_workspace_bytes(n, sum of caps) bytes
    (allocated here when None)."""
    return entropy.encode_slots(addr, caps, bound, lambda n, total, slots, off, cap, dst_len, w: L.check(L.lib().rpcc_deflate_encode(
        ptr(addr), ptr(lens), n, total, ptr(slots), ptr(off), ptr(cap), ptr(dst_len), ptr(w), stream())),
        work_bytes=lambda n, total: L.lib().rpcc_deflate_workspace_bytes(n, total), ws=ws)


def compress_many(buffers, device=None, ws=None):
    """[bytes-like or numpy array] -> [gzip member bytes]: one H2D copy, the launches, one D2H copy."""
    if not buffers:
        return []
    got, body, off = entropy.encode_list([entropy.as_bytes(b) for b in buffers], device, encode_descriptors, ws=ws)
    if (got < 0).any():
        raise RuntimeError("rpcc_deflate_encode: a stream was refused (length out of range)")
    return [body[o: o + g].tobytes() for o, g in zip(off, got)]


def compress(buffer):
    """gzip.compress's form: one gzip member."""
    return compress_many([buffer])[0]
