"""The gzip back-end of basic_compressor 'deflate' / 'gzip' on the device (librpcc_deflate.so).

compress() gives one gzip member, as gzip.compress does: other bytes (the parse and the code lengths are the build's own), the
same format, so gzip.decompress -- the reference's decoder -- reads it, and so does inflate_codec on the device.  compress_many codes a
list with one copy to the device, the launches and one copy back; encode_descriptors is the device form the batch pipeline
uses, and lz4_codec.pack_containers compacts its output into .rpcc containers."""
import numpy as np
import torch

from . import _deflate_lib as L
from ._lib import ptr, stream
from .lz4_codec import _as_bytes, _device, _upload


def bound(n):
    """Worst-case bytes of compress() for n input bytes: header, trailer and stored blocks of at most 65535 bytes."""
    return 18 + n + 5 * max(1, -(-n // 65535))


def encode_descriptors(addr, lens, caps, ws=None):
    """Device form of compress over descriptors: addr, lens (i64 GPU tensors [n]) the streams' device addresses and byte counts,
    caps (host ints) an upper bound of each length.  Enqueued on the current stream, nothing waited for.  -> (slots u8, dst_off i64,
    dst_len i64 GPU tensors, dst_off as numpy): stream s as a gzip member at slots[dst_off[s]:][:dst_len[s]], dst_len[s] < 0 when
    its length was out of range or above its cap.  ws: the caller's work buffer of rpcc_deflate_workspace_bytes(n, sum of caps) bytes
    (allocated here when None)."""
    dev = addr.device
    cap = np.array([bound(int(c)) for c in caps], np.int64)
    off = np.zeros(len(cap), np.int64)
    off[1:] = np.cumsum(cap)[:-1]
    meta = torch.from_numpy(np.stack([off, cap])).to(dev, non_blocking=True)
    slots = torch.empty(max(int(cap.sum()), 1), dtype=torch.uint8, device=dev)
    dst_len = torch.empty(len(cap), dtype=torch.int64, device=dev)
    if len(cap):
        total = int(sum(int(c) for c in caps))
        if ws is None:
            ws = torch.empty(max(L.lib().rpcc_deflate_workspace_bytes(len(cap), total), 8) // 8 + 1, dtype=torch.int64, device=dev)
        L.check(L.lib().rpcc_deflate_encode(ptr(addr), ptr(lens), len(cap), total, ptr(slots), ptr(meta[0]), ptr(meta[1]), ptr(dst_len),
                                            ptr(ws), stream()))
    return slots, meta[0], dst_len, off


def compress_many(buffers, device=None, ws=None):
    """[bytes-like or numpy array] -> [gzip member bytes]: one H2D copy, the launches, one D2H copy."""
    if not buffers:
        return []
    dev = _device(device)
    arrays = [_as_bytes(b) for b in buffers]
    with torch.cuda.device(dev):
        data, offs = _upload(arrays, dev)
        sizes = [a.size for a in arrays]
        desc = torch.tensor([[data.data_ptr() + int(o) for o in offs], sizes], dtype=torch.int64).to(dev, non_blocking=True)
        slots, _, dst_len, off = encode_descriptors(desc[0], desc[1], sizes, ws=ws)
        # [dst_len as bytes | slots] leave in one copy
        both = torch.cat([dst_len.view(torch.uint8), slots]).cpu().numpy()
        torch.cuda.current_stream(dev).synchronize()
    n = len(arrays)
    got = both[: 8 * n].view(np.int64)
    if (got < 0).any():
        raise RuntimeError("rpcc_deflate_encode: a stream was refused (length out of range)")
    body = both[8 * n:]
    return [body[o: o + g].tobytes() for o, g in zip(off, got)]


def compress(buffer):
    """gzip.compress's form: one gzip member."""
    return compress_many([buffer])[0]
