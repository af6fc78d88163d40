"""tests/deflate_ref.py, the Python statement of DESIGN.md section 12: its streams are gzip members the standard library
reads, its codes are complete and within their limits, and its sizes are the pinned ones.  No GPU needed."""
import gzip
import os
import struct
import sys
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import deflate_cases as cases  # noqa: E402
import deflate_ref as D  # noqa: E402
import lz4_ref  # noqa: E402

UNIFORM = ("contour_map", "idx_sequence", "plane_param", "q_uniform")


def all_inputs():
    return dict(cases.golden_arrays(), **cases.edge_inputs())


def test_round_trip_and_framing():
    for name, src in all_inputs().items():
        ref = cases.reference(name)
        assert gzip.decompress(ref) == src, name
        assert ref[:10] == bytes([0x1F, 0x8B, 8, 0, 0, 0, 0, 0, 0, 0xFF]), name
        assert ref[-8:] == struct.pack("<II", zlib.crc32(src), len(src) & 0xFFFFFFFF), name
        d = zlib.decompressobj(-15)
        assert d.decompress(ref[10:-8]) + d.flush() == src and d.eof and d.unused_data == b"", name
        assert len(ref) <= D.bound(len(src)), name
    assert cases.reference("len0")[10:-8] == bytes([1, 0, 0, 0xFF, 0xFF])


def test_code_lengths_complete_and_limited():
    for name, src in all_inputs().items():
        t = D.tables(src)
        for lens, maxbits in ((t["ll"], 15), (t["dl"], 15), (t["cl"], 7)):
            used = [x for x in lens if x]
            assert len(used) >= 2 and max(used) <= maxbits, name
            assert sum(1 << (maxbits - x) for x in used) == 1 << maxbits, name
        assert t["ll"][256] > 0 and 257 <= t["hlit"] <= 286 and 1 <= t["hdist"] <= 30 and 4 <= t["hclen"] <= 19, name
    # a stream without matches: distance codes 0 and 1, one bit each
    t = D.tables(cases.edge_inputs()["len11"])
    assert t["dl"][:2] == [1, 1] and not any(t["dl"][2:]) and t["hdist"] == 2


def test_length_limit_is_reached():
    """The Fibonacci frequencies give a tree deeper than 15 before the limit: the limited code uses 15-bit codes."""
    t = D.tables(cases.edge_inputs()["fibonacci"])
    assert max(t["ll"]) == 15
    fib = [1, 1]
    while len(fib) < 24:
        fib.append(fib[-1] + fib[-2])
    assert max(D.code_lengths(fib, 32)) == 23 and max(D.code_lengths(fib, 15)) == 15
    assert sum(1 << (15 - x) for x in D.code_lengths(fib, 15)) == 1 << 15


def test_split_rule():
    want = {264: [258], 265: [256, 3], 266: [257, 3], 267: [258, 3], 268: [258, 4]}
    for n, lens in want.items():
        for more in (0, 1):   # 522 .. 526: the same behind one more 258
            kind, va, vb = D.symbols(bytes(n + 258 * more))
            assert va[kind == 1].tolist() == [258] * more + lens, n
            assert (vb[kind == 1] == 1).all()
    for L in range(3, 1600):
        s = D.split(L)
        assert sum(s) == L and min(s) >= 3 and max(s) <= 258 and len(s) == -(-L // 258), L
    kind, va, _ = D.symbols(bytes(300000))
    assert int((kind == 1).sum()) == 1163


def test_window():
    """A copy 32768 bytes back is matched, one 32769 bytes back is not."""
    kind, va, vb = D.symbols(cases.edge_inputs()["offset_32768"])
    assert 32768 in vb[kind == 1].tolist()
    kind, va, vb = D.symbols(cases.edge_inputs()["offset_32769"])
    assert vb[kind == 1].max() <= 32768 and 32769 not in vb.tolist()
    assert len(cases.reference("offset_32769")) < len(cases.reference("offset_32768")) < 200


def test_long_literal_run():
    seqs, _ = D.sequences(cases.edge_inputs()["long_literals"])
    assert max(ll for _, ll, _, _ in seqs) >= 2000


def test_pinned_sizes():
    for name, size in cases.PINNED.items():
        assert len(cases.reference(name)) == size, name


def test_not_larger_than_lz4():
    for name, src in cases.golden_arrays().items():
        assert len(cases.reference(name)) <= len(lz4_ref.dumps(src)), name


def test_smaller_than_zlib_level_1():
    arrays = cases.golden_arrays()
    ours = sum(len(cases.reference(k)) for k in UNIFORM)
    theirs = sum(len(zlib.compress(arrays[k], 1)) for k in UNIFORM)
    assert ours < theirs, (ours, theirs)


def test_random_bytes_are_stored():
    for name, blocks in (("random_65535", 1), ("random_65536", 2), ("random_70000", 2)):
        src = cases.edge_inputs()[name]
        ref = cases.reference(name)
        assert len(ref) == 18 + len(src) + 5 * blocks <= D.bound(len(src)), name
        assert ref[10] == (1 if blocks == 1 else 0) and ref[10: 10 + 5] == D.stored(src)[:5], name
    for n in (0, 1, 65535, 65536, 131070, 131071, 188106):
        assert D.bound(n) == 18 + n + 5 * max(1, -(-n // 65535))


def test_exact_fit_stays_dynamic():
    """A dynamic block of exactly the stored size, in whole bytes, is still taken, and the member is bound(n) long."""
    src = cases.edge_inputs()["exact_fit"]
    ref = cases.reference("exact_fit")
    assert D.dynamic_block(src)[1] == 8 * (len(src) + 5)
    assert ref[10] & 7 == 5 and len(ref) == D.bound(len(src))
