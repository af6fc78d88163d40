"""The LZ4 back-end of basic_compressor 'lz4' on the device (librpcc_lz4.so).

dumps / loads are python-lz4 0.7.0's names and forms: a uint32 little-endian uncompressed size, then one raw LZ4 block; the
blocks are valid LZ4, so liblz4 or the reference's lz4.loads reads them, and loads reads any LZ4 block.  compress_utils takes
this module where the lz4 package is not installed.  dumps_many / loads_many code a list with one copy to the device, one
launch and one copy back; encode_descriptors / pack_containers / decode_descriptors are the device forms the batch pipelines use."""
import struct

import numpy as np
import torch

from . import _lz4_lib as L
from . import entropy
from ._lib import ptr, stream

_STATUS = {L.E_CAPACITY: "header size larger than the output capacity", L.E_TRUNCATED: "truncated header, token, literal or offset",
           L.E_OFFSET: "offset 0 or before the start of the output", L.E_OVERRUN: "output overrun (more bytes than the header says)",
           L.E_SIZE: "produced size differs from the header"}


def bound(n):
    """Worst-case bytes of dumps() for n input bytes."""
    return 4 + n + n // 255 + 16


def encode_descriptors(addr, lens, caps):
    """Device form of dumps over descriptors: addr, lens (i64 GPU tensors [n]) the streams' device addresses and byte counts, caps
    (host ints) an upper bound of each length.  Enqueued on the current stream, nothing waited for.  -> (slots u8, dst_off i64,
    dst_len i64 GPU tensors, dst_off as numpy): stream s in dumps form at slots[dst_off[s]:][:dst_len[s]], dst_len[s] < 0 when its
    length was out of range."""
    return entropy.encode_slots(addr, caps, bound, lambda n, total, slots, off, cap, dst_len, ws: L.check(L.lib().rpcc_lz4_encode(
        ptr(addr), ptr(lens), n, ptr(slots), ptr(off), ptr(cap), ptr(dst_len), stream())))


def encode_tensors(srcs):
    """encode_descriptors over contiguous GPU tensors (any dtype, read as bytes)."""
    for t in srcs:
        if not t.is_cuda or not t.is_contiguous():
            raise ValueError("encode_tensors: expects contiguous GPU tensors")
    nbytes = [t.numel() * t.element_size() for t in srcs]
    dev = entropy.device_of(None)
    desc = torch.tensor([[t.data_ptr() for t in srcs], nbytes], dtype=torch.int64).to(dev, non_blocking=True)
    return encode_descriptors(desc[0], desc[1], nbytes)


def pack_containers(slots, dst_off, dst_len, nframes, per_frame, out_cap, ws=None):
    """The .rpcc containers of nframes frames of per_frame streams (encode_tensors' output, frame-major) back to back on the device.
    ws: the caller's work buffer of rpcc_lz4_workspace_bytes(nframes * per_frame) bytes (allocated here when None).
    -> (out u8, frame i64 [2, nframes]: offsets and lengths, -1 for a frame that failed)."""
    dev = slots.device
    out = torch.empty(max(int(out_cap), 1), dtype=torch.uint8, device=dev)
    frame = torch.empty((2, max(nframes, 1)), dtype=torch.int64, device=dev)
    if ws is None:
        ws = torch.empty(max(L.lib().rpcc_lz4_workspace_bytes(nframes * per_frame), 8), dtype=torch.uint8, device=dev)
    L.check(L.lib().rpcc_lz4_pack_containers(ptr(slots), ptr(dst_off), ptr(dst_len), nframes, per_frame, ptr(out), int(out_cap),
                                             ptr(frame[0]), ptr(frame[1]), ptr(ws), stream()))
    return out, frame


def dumps_many(buffers, device=None):
    """[bytes-like or numpy array] -> [dumps form bytes]: one H2D copy, one launch, one D2H copy."""
    if not buffers:
        return []
    got, body, off = entropy.encode_list([entropy.as_bytes(b) for b in buffers], device, encode_descriptors)
    if (got < 0).any():
        raise RuntimeError("rpcc_lz4_encode: a stream was refused (length out of range)")
    return [body[o: o + g].tobytes() for o, g in zip(off, got)]


def decode_descriptors(addr, lens, dst, dst_off, dst_cap):
    """Device form of loads over descriptors: stream s reads lens[s] bytes (dumps form) at the device address addr[s] and is written at
    dst[dst_off[s]:], at most dst_cap[s] bytes (addr, lens, dst_off, dst_cap: i64 GPU tensors [n]; dst: u8 GPU tensor).  Enqueued on the
    current stream, nothing waited for.  -> (dst_len i64 [n], status i32 [n]) GPU tensors."""
    n = addr.numel()
    dst_len = torch.empty(n, dtype=torch.int64, device=addr.device)
    status = torch.empty(n, dtype=torch.int32, device=addr.device)
    if n:
        L.check(L.lib().rpcc_lz4_decode(ptr(addr), ptr(lens), n, ptr(dst), ptr(dst_off), ptr(dst_cap), ptr(dst_len), ptr(status), stream()))
    return dst_len, status


def decode_many(blobs, device=None):
    """[dumps form bytes] -> (status int32 [n]: 0 or RPCC_LZ4_E_*, [bytes]): one H2D copy, one launch, one D2H copy."""
    if not blobs:
        return np.zeros(0, np.int32), []
    arrays = [entropy.as_bytes(b) for b in blobs]
    # the header is on the host: size each output by it, but never beyond what a valid block of that length can produce (255:1)
    cap = np.array([min(struct.unpack_from("<I", a)[0], 255 * a.size) if a.size >= 4 else 0 for a in arrays], np.int64)
    res = entropy.decode_list(arrays, cap, entropy.device_of(device), lambda n, m, out, cols, status, work: L.check(L.lib().rpcc_lz4_decode(
        ptr(m[0]), ptr(m[1]), n, ptr(out), ptr(m[2]), ptr(m[3]), ptr(cols[0]), ptr(status), stream())))
    return res[0], entropy.slot_bytes(*res)


def loads_many(blobs, device=None):
    """[dumps form bytes] -> [bytes].  ValueError names the first bad stream."""
    st, outs = decode_many(blobs, device)
    entropy.raise_first_bad(st, "lz4", _STATUS)
    return outs


def dumps(buffer):
    """python-lz4 0.7.0's lz4.dumps: uint32 LE size + one LZ4 block."""
    return dumps_many([buffer])[0]


def loads(data):
    """python-lz4 0.7.0's lz4.loads; ValueError on a bad stream."""
    return loads_many([data])[0]

