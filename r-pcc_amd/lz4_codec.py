"""The LZ4 back-end of basic_compressor 'lz4' on the device (librpcc_lz4.so).

dumps / loads are python-lz4 0.7.0's names and forms: a uint32 little-endian uncompressed size, then one raw LZ4 block; the
blocks are valid LZ4, so liblz4 or the reference's lz4.loads reads them, and loads reads any LZ4 block.  compress_utils takes
this module where the lz4 package is not installed.  dumps_many / loads_many code a list with one copy to the device, one
launch and one copy back; encode_descriptors / pack_containers / decode_descriptors are the device forms the batch pipelines use."""
import struct

import numpy as np
import torch

from . import _lz4_lib as L
from ._lib import ptr, stream

_STATUS = {L.E_CAPACITY: "header size larger than the output capacity", L.E_TRUNCATED: "truncated header, token, literal or offset",
           L.E_OFFSET: "offset 0 or before the start of the output", L.E_OVERRUN: "output overrun (more bytes than the header says)",
           L.E_SIZE: "produced size differs from the header"}


def bound(n):
    """Worst-case bytes of dumps() for n input bytes."""
    return 4 + n + n // 255 + 16


def _device(device):
    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


def _as_bytes(buf):
    if isinstance(buf, np.ndarray):
        return np.ascontiguousarray(buf).view(np.uint8).reshape(-1)
    return np.frombuffer(memoryview(buf).cast("B"), np.uint8)


def _upload(arrays, device):
    """The arrays in one pinned host buffer, each at an 8-byte aligned offset -> one H2D copy.  -> (device tensor, payload offsets)."""
    offs = np.zeros(len(arrays) + 1, np.int64)
    offs[1:] = np.cumsum([(a.size + 7) // 8 * 8 for a in arrays])
    host = torch.empty(int(offs[-1]), dtype=torch.uint8, pin_memory=True)
    h = host.numpy()
    for a, o in zip(arrays, offs[:-1]):
        h[o: o + a.size] = a
    return host.to(device, non_blocking=True), offs[:-1]


def encode_descriptors(addr, lens, caps):
    """Device form of dumps over descriptors: addr, lens (i64 GPU tensors [n]) the streams' device addresses and byte counts, caps
    (host ints) an upper bound of each length.  Enqueued on the current stream, nothing waited for.  -> (slots u8, dst_off i64,
    dst_len i64 GPU tensors, dst_off as numpy): stream s in dumps form at slots[dst_off[s]:][:dst_len[s]], dst_len[s] < 0 when its
    length was out of range."""
    dev = addr.device
    cap = np.array([bound(int(c)) for c in caps], np.int64)
    off = np.zeros(len(cap), np.int64)
    off[1:] = np.cumsum(cap)[:-1]
    meta = torch.from_numpy(np.stack([off, cap])).to(dev, non_blocking=True)
    slots = torch.empty(max(int(cap.sum()), 1), dtype=torch.uint8, device=dev)
    dst_len = torch.empty(len(cap), dtype=torch.int64, device=dev)
    if len(cap):
        L.check(L.lib().rpcc_lz4_encode(ptr(addr), ptr(lens), len(cap), ptr(slots), ptr(meta[0]), ptr(meta[1]), ptr(dst_len), stream()))
    return slots, meta[0], dst_len, off


def encode_tensors(srcs):
    """encode_descriptors over contiguous GPU tensors (any dtype, read as bytes)."""
    for t in srcs:
        if not t.is_cuda or not t.is_contiguous():
            raise ValueError("encode_tensors: expects contiguous GPU tensors")
    nbytes = [t.numel() * t.element_size() for t in srcs]
    dev = _device(None)
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
    dev = _device(device)
    arrays = [_as_bytes(b) for b in buffers]
    with torch.cuda.device(dev):
        data, offs = _upload(arrays, dev)
        sizes = [a.size for a in arrays]
        desc = torch.tensor([[data.data_ptr() + int(o) for o in offs], sizes], dtype=torch.int64).to(dev, non_blocking=True)
        slots, _, dst_len, off = encode_descriptors(desc[0], desc[1], sizes)
        # [dst_len as bytes | slots] leave in one copy
        both = torch.cat([dst_len.view(torch.uint8), slots]).cpu().numpy()
        torch.cuda.current_stream(dev).synchronize()
    n = len(arrays)
    got = both[: 8 * n].view(np.int64)
    if (got < 0).any():
        raise RuntimeError("rpcc_lz4_encode: a stream was refused (length out of range)")
    body = both[8 * n:]
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
    dev = _device(device)
    arrays = [_as_bytes(b) for b in blobs]
    # the header is on the host: size each output by it, but never beyond what a valid block of that length can produce (255:1)
    cap = np.array([min(struct.unpack_from("<I", a)[0], 255 * a.size) if a.size >= 4 else 0 for a in arrays], np.int64)
    off = np.zeros(len(cap), np.int64)
    off[1:] = np.cumsum((cap + 7) // 8 * 8)[:-1]
    n = len(arrays)
    with torch.cuda.device(dev):
        data, doffs = _upload(arrays, dev)
        addr = np.array([data.data_ptr() + int(o) for o in doffs], np.uint64).view(np.int64)
        meta = torch.from_numpy(np.stack([addr, np.array([a.size for a in arrays], np.int64), off, cap])).to(dev, non_blocking=True)
        res = torch.empty(16 * n + max(int(off[-1] + cap[-1]), 1), dtype=torch.uint8, device=dev)   # [dst_len | status | pad | bytes]
        dst_len, status, out = res[: 8 * n].view(torch.int64), res[8 * n: 12 * n].view(torch.int32), res[16 * n:]
        L.check(L.lib().rpcc_lz4_decode(ptr(meta[0]), ptr(meta[1]), n, ptr(out), ptr(meta[2]), ptr(meta[3]), ptr(dst_len), ptr(status),
                                        stream()))
        h = res.cpu().numpy()
    lens, st, body = h[: 8 * n].view(np.int64), h[8 * n: 12 * n].view(np.int32).copy(), h[16 * n:]
    return st, [body[o: o + l].tobytes() if s == 0 else None for o, l, s in zip(off, lens, st)]


def loads_many(blobs, device=None):
    """[dumps form bytes] -> [bytes].  ValueError names the first bad stream."""
    st, outs = decode_many(blobs, device)
    bad = np.flatnonzero(st != L.OK)
    if bad.size:
        k = int(bad[0])
        raise ValueError("lz4 stream %d: %s (status %d)" % (k, _STATUS.get(int(st[k]), "error"), int(st[k])))
    return outs


def dumps(buffer):
    """python-lz4 0.7.0's lz4.dumps: uint32 LE size + one LZ4 block."""
    return dumps_many([buffer])[0]


def loads(data):
    """python-lz4 0.7.0's lz4.loads; ValueError on a bad stream."""
    return loads_many([data])[0]

