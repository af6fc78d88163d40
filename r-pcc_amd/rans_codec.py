"""The back-end of basic_compressor 'rans' (librpcc_rans.so): an order-0 rANS coder over fixed-size chunks, 64
interleaved states per chunk and a directory of chunk lengths per stream, so that every chunk of every stream of a batch is coded by a
wavefront of its own.  The format is the build's own: there is no host coder in the product, the reference project cannot read these
streams, and a machine without a GPU cannot either.

A stream carries its element width (1, 2 or 4: byte i belongs to plane i mod width, every plane has its own frequency table), which the
callers take from the arrays they code.  A stream may also be coded through the delta filter (format version 2, magic 'RB':
the zigzagged differences of consecutive elements, each chunk on its own), which the encoders take as filters= beside widths=;
delta_filter() is the one rule for which arrays get it when a caller asks for the filter (rans_delta).  The decoders read both versions
and take no option.  compress_many / decompress_many code a list with one copy to the device, the launches and one
copy back; encode_descriptors / encode_tensors / decode_descriptors are the device forms the batch pipelines use.  Importing this module
touches neither the device nor the library."""
import struct

import numpy as np
import torch

from . import _rans_lib as L
from . import entropy
from ._lib import ptr, stream

HEADER = 12
FILTER_NONE, FILTER_DELTA = L.FILTER_NONE, L.FILTER_DELTA
_STATUS = {L.E_CAPACITY: "header size larger than the output capacity", L.E_HEADER: "bad magic, mode, width, chunk size, filter or reserved bytes",
           L.E_TRUNCATED: "truncated header, table or directory", L.E_TABLE: "a frequency table is out of order or does not sum to 4096",
           L.E_DIRECTORY: "the chunk lengths do not end at the end of the stream", L.E_STATE: "a chunk ends in a wrong state or with words left over",
           L.E_PAYLOAD: "a chunk reads past its payload"}


def bound(n):
    """Worst-case bytes of a stream of n input bytes: the stored form."""
    return HEADER + n


def delta_filter(dtype):
    """The filter of an array of this dtype when the delta filter is asked for (rans_delta): signed 16-bit arrays -- the quantised
    residuals, whose neighbours differ by a step or less most of the time -- get it, everything else gets none: on the example sweep the
    filter takes the residuals from 86 621 to 30 222 bytes and makes the contour bits, the index sequence and the model rows larger
    (DESIGN.md section 19)."""
    return FILTER_DELTA if dtype is not None and np.dtype(dtype) == np.int16 else FILTER_NONE


def encode_descriptors(addr, lens, caps, widths=None, chunk_log2=None, ws=None, filters=None):
    """Device form of compress over descriptors: addr, lens (i64 GPU tensors [n]) the streams' device addresses and byte counts, caps (host
    ints) an upper bound of each length, widths (host ints 1 / 2 / 4, one per stream; None: 1) their element sizes, filters (host ints
    FILTER_NONE / FILTER_DELTA, one per stream; None: no filter) -- a filtered stream that would not shrink comes out as the version-1
    stored stream.  Enqueued on the
    current stream, nothing waited for.  -> (slots u8, dst_off i64, dst_len i64 GPU tensors, dst_off as numpy): stream s at
    slots[dst_off[s]:][:dst_len[s]], dst_len[s] < 0 when its length was out of range or above its cap.  ws: the caller's work buffer of
    rpcc_rans_workspace_bytes(n, sum of caps, chunk_log2) bytes (allocated here when None)."""
    clog = L.DEFAULT_CHUNK_LOG2 if chunk_log2 is None else int(chunk_log2)
    wd = None
    if (widths is not None or filters is not None) and len(caps):
        words = np.ones(len(caps), np.int32) if widths is None else np.asarray(widths, np.int32).reshape(len(caps))
        if filters is not None:      # RPCC_RANS_WIDTH_WORD
            words = words | np.asarray(filters, np.int32).reshape(len(caps)) << 8
        wd = torch.from_numpy(words).to(addr.device, non_blocking=True)

    def work_bytes(n, total):
        nbytes = L.lib().rpcc_rans_workspace_bytes(n, total, clog)
        if nbytes == 0:
            raise ValueError("rpcc_rans_workspace_bytes(%d, %d, %d): out of range (chunk_log2 8 .. 16)" % (n, total, clog))
        return nbytes
    return entropy.encode_slots(addr, caps, bound, lambda n, total, slots, off, cap, dst_len, w: L.check(L.lib().rpcc_rans_encode(
        ptr(addr), ptr(lens), ptr(wd), n, total, clog, ptr(slots), ptr(off), ptr(cap), ptr(dst_len), ptr(w), stream())),
        work_bytes=work_bytes, align=16, ws=ws)


def encode_tensors(srcs, chunk_log2=None, filters=None):
    """encode_descriptors over contiguous GPU tensors, each coded at its element size (1, 2 or 4 bytes; wider elements as bytes)."""
    for t in srcs:
        if not t.is_cuda or not t.is_contiguous():
            raise ValueError("encode_tensors: expects contiguous GPU tensors")
    nbytes = [t.numel() * t.element_size() for t in srcs]
    dev = entropy.device_of(None)
    desc = torch.tensor([[t.data_ptr() for t in srcs], nbytes], dtype=torch.int64).to(dev, non_blocking=True)
    return encode_descriptors(desc[0], desc[1], nbytes, widths=[_width(t.element_size()) for t in srcs], chunk_log2=chunk_log2, filters=filters)


def _width(itemsize):
    return itemsize if itemsize in (1, 2, 4) else 1


def compress_many(buffers, device=None, chunk_log2=None, filters=None):
    """[bytes-like or numpy array] -> [stream bytes]: an array is coded at its itemsize, anything else as bytes; filters as for
    encode_descriptors (None: version-1 streams)."""
    if not buffers:
        return []
    widths = [_width(b.itemsize) if isinstance(b, np.ndarray) else 1 for b in buffers]
    kw = {} if filters is None else dict(filters=filters)
    got, body, off = entropy.encode_list([entropy.as_bytes(b) for b in buffers], device, encode_descriptors, widths=widths, chunk_log2=chunk_log2, **kw)
    if (got < 0).any():
        raise RuntimeError("rpcc_rans_encode: a stream was refused (length out of range)")
    return [body[o: o + g].tobytes() for o, g in zip(off, got)]


def compress_many_delta(buffers, device=None, chunk_log2=None):
    """compress_many with the delta filter on the arrays delta_filter() names: what BasicCompressor(..., rans_delta=True) codes with."""
    return compress_many(buffers, device, chunk_log2, filters=[delta_filter(b.dtype if isinstance(b, np.ndarray) else None) for b in buffers])


def decode_descriptors(addr, lens, dst, dst_off, dst_cap):
    """Device form of decompress over descriptors (streams of either version): stream s reads lens[s] bytes at the device address addr[s] and is written at
    dst[dst_off[s]:], at most dst_cap[s] bytes (addr, lens, dst_off, dst_cap: i64 GPU tensors [n]; dst: u8 GPU tensor).  Enqueued on the
    current stream, nothing waited for.  -> (dst_len i64 [n], status i32 [n]) GPU tensors; a refused stream's slot is left as it was."""
    n = addr.numel()
    dst_len = torch.empty(n, dtype=torch.int64, device=addr.device)
    status = torch.empty(n, dtype=torch.int32, device=addr.device)
    if n:
        L.check(L.lib().rpcc_rans_decode(ptr(addr), ptr(lens), n, ptr(dst), ptr(dst_off), ptr(dst_cap), ptr(dst_len), ptr(status), stream()))
    return dst_len, status


def decode_many(blobs, device=None):
    """[stream bytes] -> (status int32 [n]: 0 or RPCC_RANS_E_*, [bytes or None])."""
    if not blobs:
        return np.zeros(0, np.int32), []
    arrays = [entropy.as_bytes(b) for b in blobs]
    # n is on the host, at header offset 4: size each output by it, but never beyond what a valid stream of that length can hold (a chunk
    # of up to 2^16 bytes takes 4 directory bytes and 256 of states at least: below 256:1)
    cap = np.array([min(struct.unpack_from("<I", a, 4)[0], 256 * a.size) if a.size >= HEADER else 0 for a in arrays], np.int64)
    res = entropy.decode_list(arrays, cap, entropy.device_of(device), lambda n, m, out, cols, status, work: L.check(L.lib().rpcc_rans_decode(
        ptr(m[0]), ptr(m[1]), n, ptr(out), ptr(m[2]), ptr(m[3]), ptr(cols[0]), ptr(status), stream())))
    return res[0], entropy.slot_bytes(*res)


def decompress_many(blobs, device=None):
    """[stream bytes] -> [bytes].  ValueError names the first bad stream."""
    st, outs = decode_many(blobs, device)
    entropy.raise_first_bad(st, "rans", _STATUS)
    return outs


def compress(buffer):
    return compress_many([buffer])[0]


def decompress(data):
    return decompress_many([data])[0]
