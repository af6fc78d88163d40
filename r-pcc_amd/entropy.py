"""What the device entropy back-ends share on the host (DESIGN.md sections 11-15, 19): staging a list of byte strings on the device, the
slot layouts, the list drivers of the encoders and of the decoders, and the error of the first bad stream.  lz4_codec, deflate_codec,
bzip2_codec, inflate_codec, bunzip2_codec and rans_codec keep what is their format's: bounds, status texts, sizing, retries and host fallbacks."""
import numpy as np
import torch


def device_of(device):
    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


def as_bytes(buf):
    if isinstance(buf, np.ndarray):
        return np.ascontiguousarray(buf).view(np.uint8).reshape(-1)
    return np.frombuffer(memoryview(buf).cast("B"), np.uint8)


def packed_slots(sizes):
    """Slots back to back, no padding (the encoders' output, which pack_containers relies on).  -> (offsets i64 [n], total bytes)."""
    sizes = np.asarray(sizes, np.int64).reshape(-1)
    end = np.cumsum(sizes)
    return end - sizes, int(end[-1]) if sizes.size else 0


def aligned_slots(sizes):
    """Slots that each start at an 8-byte multiple (staged inputs, the decoders' outputs and work slots).  -> (offsets i64 [n], the end of
    the last slot: its own size is not rounded up)."""
    sizes = np.asarray(sizes, np.int64).reshape(-1)
    off = packed_slots((sizes + 7) // 8 * 8)[0]
    return off, int(off[-1] + sizes[-1]) if sizes.size else 0


def upload(arrays, device):
    """The arrays in one pinned host buffer, each at an 8-byte aligned offset -> one H2D copy.  -> (device tensor, payload offsets)."""
    offs, end = aligned_slots([a.size for a in arrays])
    host = torch.empty((end + 7) // 8 * 8, dtype=torch.uint8, pin_memory=True)
    h = host.numpy()
    for a, o in zip(arrays, offs):
        h[o: o + a.size] = a
    return host.to(device, non_blocking=True), offs


def work_buffer(nbytes, align, device):
    """A work buffer of nbytes bytes at an address that is a multiple of align (8 or 16)."""
    ws = torch.empty(max(nbytes, align) // 8 + align // 8, dtype=torch.int64, device=device)
    return ws[(-ws.data_ptr() // 8) % (align // 8):]


def encode_slots(addr, caps, bound, launch, work_bytes=None, align=8, ws=None):
    """The body of a back-end's encode_descriptors: a slot of bound(cap) bytes for each stream, back to back, and one call of the library.
    launch(n, total, slots, dst_off, dst_cap, dst_len, ws): the ABI call over GPU tensors (total: the sum of caps); work_bytes(n, total): the
    library's work buffer size, allocated here at a multiple of align when the caller brings no ws (None: the library takes none).
    -> (slots u8, dst_off i64, dst_len i64 GPU tensors, dst_off as numpy)."""
    dev = addr.device
    cap = np.array([bound(int(c)) for c in caps], np.int64)
    off, nbytes = packed_slots(cap)
    meta = torch.from_numpy(np.stack([off, cap])).to(dev, non_blocking=True)
    slots = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    dst_len = torch.empty(len(cap), dtype=torch.int64, device=dev)
    if len(cap):
        total = int(sum(int(c) for c in caps))
        if ws is None and work_bytes is not None:
            ws = work_buffer(work_bytes(len(cap), total), align, dev)
        launch(len(cap), total, slots, meta[0], meta[1], dst_len, ws)
    return slots, meta[0], dst_len, off


def encode_list(arrays, device, encode_descriptors, **kw):
    """The list encoders' driver: one H2D copy, encode_descriptors(addr, lens, caps, **kw), one D2H copy of [dst_len as bytes | slots].
    -> (dst_len i64 [n], the slots' bytes, their offsets) on the host."""
    dev = device_of(device)
    with torch.cuda.device(dev):
        data, offs = upload(arrays, dev)
        sizes = [a.size for a in arrays]
        desc = torch.tensor([[data.data_ptr() + int(o) for o in offs], sizes], dtype=torch.int64).to(dev, non_blocking=True)
        slots, _, dst_len, off = encode_descriptors(desc[0], desc[1], sizes, **kw)
        both = torch.cat([dst_len.view(torch.uint8), slots]).cpu().numpy()
        torch.cuda.current_stream(dev).synchronize()
    n = len(arrays)
    return both[: 8 * n].view(np.int64), both[8 * n:], off


def decode_list(arrays, cap, device, launch, work_cap=None, extra=0):
    """The list decoders' launch: one H2D copy, one launch, one D2H copy.  cap: the output slots' sizes; work_cap: the work slots' sizes
    where the back-end has them; extra: int64 result columns beside dst_len.  launch(n, meta, out, cols, status, work): the ABI call over
    GPU tensors -- meta i64 rows [addr | lens | dst_off | dst_cap (| work_off | work_cap)], cols i64 [1 + extra, n] with dst_len first.
    -> (status i32 [n], dst_len i64 [n], the slots' bytes, their offsets) on the host."""
    n = len(arrays)
    off, end = aligned_slots(cap)
    rows = [np.array([a.size for a in arrays], np.int64), off, cap]
    if work_cap is not None:
        woff, wend = aligned_slots(work_cap)
        rows += [woff, work_cap]
    with torch.cuda.device(device):
        data, doffs = upload(arrays, device)
        addr = np.array([data.data_ptr() + int(o) for o in doffs], np.uint64).view(np.int64)
        meta = torch.from_numpy(np.stack([addr] + rows)).to(device, non_blocking=True)
        work = None if work_cap is None else torch.empty(max(wend, 8), dtype=torch.uint8, device=device)
        ncol, head = 8 * n * (1 + extra), 8 * n * (2 + extra)
        res = torch.empty(head + max(end, 1), dtype=torch.uint8, device=device)   # [dst_len | extra columns | status | pad | bytes]
        launch(n, meta, res[head:], res[:ncol].view(torch.int64).view(1 + extra, n), res[ncol: ncol + 4 * n].view(torch.int32), work)
        h = res.cpu().numpy()
    return h[ncol: ncol + 4 * n].view(np.int32).copy(), h[: 8 * n].view(np.int64), h[head:], off


def slot_bytes(status, dst_len, body, off):
    """decode_list's result as a list: the bytes of every stream whose status is 0, None for the others."""
    return [body[o: o + l].tobytes() if s == 0 else None for o, l, s in zip(off, dst_len, status)]


def raise_first_bad(status, name, texts):
    """ValueError that names the first stream whose status is not 0.  name: what the back-end calls its streams; texts: status -> text."""
    bad = np.flatnonzero(status != 0)
    if bad.size:
        k = int(bad[0])
        raise ValueError("%s stream %d: %s (status %d)" % (name, k, texts.get(int(status[k]), "error"), int(status[k])))
