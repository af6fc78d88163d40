"""The bzip2 decoder of basic_compressor 'bzip2' on the device (librpcc_bunzip2.so).

decompress() equals bz2.decompress on every input: one bzip2 stream -- whoever wrote it -- is decoded on the GPU to the same bytes, what
bz2.decompress refuses is refused (ValueError), and the few things libbz2 reads that the kernel does not (a second stream, other
trailing bytes, a block with the randomised bit) are handed to bz2.decompress on the host.  decode_many decodes a list with one copy
to the device, one launch and one copy back where the sizes are known or guessed right; decode_descriptors is the device form: each
stream lands at an offset of the caller's choice."""
import bz2
import functools

import numpy as np
import torch

from . import _bunzip2_lib as L
from . import entropy
from ._lib import ptr, stream

GUESS_RATIO, GUESS_SLACK = 8, 4096    # a stream of n bytes is first given 8 n + 4096 bytes: this project's payloads shrink 3.4 to 6.6 times

_STATUS = {L.E_TRUNCATED: "the stream ends early", L.E_HEADER: "not a bzip2 stream (magic or level)",
           L.E_MAGIC: "neither a block nor the end of the stream", L.E_RANDOMISED: "a randomised block",
           L.E_TABLE: "invalid symbol map, group count, selector or code length", L.E_SYMBOL: "invalid code, or a run or block too long",
           L.E_ORIGPTR: "origin pointer outside the block", L.E_OVERRUN: "more output than the capacity given", L.E_CRC: "CRC mismatch",
           L.E_WORK: "a block longer than the work slot", L.E_TRAILING: "data after the stream",
           L.E_RLE: "a block ends where a run's count byte belongs"}


def status_text(st):
    return _STATUS.get(int(st), "error")


def block_bound(level, cap):
    """The longest block of a stream of this level that decodes to at most cap bytes (include/rpcc_bunzip2.h)."""
    return min(100000 * int(level), 5 * int(cap) // 4 + 8)


def work_bytes(nblock_max):
    """rpcc_bunzip2_stream_work_bytes: the work slot of a stream whose blocks hold up to nblock_max bytes."""
    v = int(L.lib().rpcc_bunzip2_stream_work_bytes(int(nblock_max)))
    if v < 0:
        L.check(v)
    return v


def decode_descriptors(addr, lens, dst, dst_off, dst_cap, work, work_off, work_cap):
    """Device form: stream s reads lens[s] bytes at the device address addr[s], is written at dst[dst_off[s]:], at most dst_cap[s] bytes,
    and uses work[work_off[s]:][:work_cap[s]] (addr, lens, dst_off, dst_cap, work_off, work_cap: i64 GPU tensors [n]; dst, work: u8 GPU
    tensors; every work slot 4-byte aligned and work_bytes(block_bound(level, cap)) long or more).  Enqueued on the current stream, nothing
    waited for.  -> (dst_len i64 [n], src_used i64 [n], status i32 [n]) GPU tensors."""
    n = addr.numel()
    dst_len = torch.empty(n, dtype=torch.int64, device=addr.device)
    src_used = torch.empty(n, dtype=torch.int64, device=addr.device)
    status = torch.empty(n, dtype=torch.int32, device=addr.device)
    if n:
        L.check(L.lib().rpcc_bunzip2_decode(ptr(addr), ptr(lens), n, ptr(dst), ptr(dst_off), ptr(dst_cap), ptr(work), ptr(work_off), ptr(work_cap),
                                            ptr(dst_len), ptr(src_used), ptr(status), stream()))
    return dst_len, src_used, status


def level_of(head):
    """The level a stream states in its fourth byte ("BZh1" .. "BZh9"); 1 for anything else, which the decoder refuses."""
    return int(head[3]) - 0x30 if len(head) > 3 and 0x31 <= int(head[3]) <= 0x39 else 1


@functools.lru_cache(maxsize=None)
def _slot_work_bytes(level, cap):
    return (work_bytes(block_bound(level, cap)) + 7) // 8 * 8


def stream_work_bytes(head, cap):
    """The work slot, an 8-byte multiple, of a stream that begins with the bytes head and decodes to at most cap bytes."""
    return _slot_work_bytes(level_of(head), int(cap))


def decode_slots(d, dst, work):
    """decode_descriptors over the descriptor rows d = [addr, lens, dst_off, dst_cap, work_off, work_cap].  -> (dst_len, status)."""
    dst_len, _, status = decode_descriptors(d[0], d[1], dst, d[2], d[3], work, d[4], d[5])
    return dst_len, status


def _launch(arrays, cap, blocks, dev):
    """One H2D copy, one launch, one D2H copy -> (status i32 [n], dst_len i64 [n], the slots' bytes, their offsets).  cap: the slots'
    sizes; blocks: the block length each work slot holds."""
    return entropy.decode_list(arrays, cap, dev, lambda n, m, out, cols, status, work: L.check(L.lib().rpcc_bunzip2_decode(
        ptr(m[0]), ptr(m[1]), n, ptr(out), ptr(m[2]), ptr(m[3]), ptr(work), ptr(m[4]), ptr(m[5]), ptr(cols[0]), ptr(cols[1]), ptr(status),
        stream())), work_cap=np.array([work_bytes(b) for b in blocks], np.int64), extra=1)


def decode_many(blobs, caps=None, device=None):
    """[bzip2 stream bytes] -> (status int32 [n]: 0 or RPCC_BUNZIP2_E_*, [bytes, None where the status is not 0]).  bzip2 states no size:
    with caps (a size for each stream, at least what it decodes to) the slots are sized from them and a stream that is longer ends in
    E_OVERRUN; without, every slot is first given GUESS_RATIO times the stream's length and GUESS_SLACK more, and a stream that ends in
    E_OVERRUN -- a complete answer, with its size -- is decoded once more at that size.  The work slots follow from the capacity and the
    level byte (block_bound); a stream that ends in E_WORK is given a work slot of its level's full block first.  One launch where the
    sizes hold, three at most.  Streams libbz2 reads and the kernel refuses (E_TRAILING, E_RANDOMISED) and the empty blob go to
    bz2.decompress on the host."""
    n = len(blobs)
    if not n:
        return np.zeros(0, np.int32), []
    dev = entropy.device_of(device)
    arrays = [entropy.as_bytes(b) for b in blobs]
    level = np.array([level_of(a) for a in arrays], np.int64)
    if caps is None:
        cap = np.array([GUESS_RATIO * a.size + GUESS_SLACK for a in arrays], np.int64)
    else:
        cap = np.maximum(np.asarray(caps, np.int64).reshape(n), 0)
    st = np.zeros(n, np.int32)
    outs = [None] * n
    todo = np.arange(n)
    blocks = np.array([block_bound(level[k], cap[k]) for k in todo], np.int64)
    for _ in range(3):
        s, lens, body, off = _launch([arrays[k] for k in todo], cap[todo], blocks, dev)
        nxt, nblocks = [], []
        for j, k in enumerate(todo):
            st[k] = s[j]
            if s[j] == L.OK:
                outs[k] = body[off[j]: off[j] + lens[j]].tobytes()
            elif s[j] == L.E_WORK and blocks[j] < 100000 * level[k]:
                nxt.append(k)
                nblocks.append(100000 * level[k])
            elif s[j] == L.E_OVERRUN and caps is None:
                cap[k] = lens[j]
                nxt.append(k)
                nblocks.append(block_bound(level[k], lens[j]))
        if not nxt:
            break
        todo, blocks = np.array(nxt), np.array(nblocks, np.int64)
    for k in range(n):
        if st[k] in (L.E_TRAILING, L.E_RANDOMISED) or arrays[k].size == 0:
            try:
                outs[k] = bz2.decompress(arrays[k].tobytes())
                st[k] = L.E_OVERRUN if caps is not None and len(outs[k]) > cap[k] else L.OK
                if st[k] != L.OK:
                    outs[k] = None
            except (OSError, ValueError, EOFError):
                pass
    return st, outs


def decompress_many(blobs, caps=None):
    """[bzip2 stream bytes] -> [bytes].  ValueError names the first bad stream."""
    st, outs = decode_many(blobs, caps)
    entropy.raise_first_bad(st, "bzip2", _STATUS)
    return outs


def decompress(blob):
    """bz2.decompress for one stream; ValueError on a bad stream."""
    return decompress_many([blob])[0]
