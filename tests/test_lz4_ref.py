"""The numpy reference of the build's LZ4 parse (tests/lz4_ref.py): the sizes of the specification's
table, round trips through the plain-Python decoder and -- where the system liblz4 loads -- LZ4_decompress_safe.  No GPU needed."""
import ctypes
import os
import struct
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import lz4_ref as R  # noqa: E402


def _liblz4():
    try:
        return ctypes.CDLL("liblz4.so.1")
    except OSError:
        return None


def _check(src):
    """dumps -> loads round trip; LZ4_decompress_safe agrees where liblz4 is there."""
    blob = R.dumps(src)
    assert R.loads(blob) == src
    lz = _liblz4()
    if lz is not None and len(src):
        out = ctypes.create_string_buffer(len(src))
        assert lz.LZ4_decompress_safe(blob[4:], out, len(blob) - 4, len(src)) == len(src)
        assert out.raw == src
    return blob


def test_table_sizes():
    """The block sizes of DESIGN.md section 11's table (the example sweep's arrays), byte for byte."""
    import gen_golden_lz4
    want = {"contour_map": 7063, "idx_sequence": 3771, "plane_param": 624, "q_uniform": 73181, "q_nonuniform": 62800, "zeros": 1187}
    for k, src in gen_golden_lz4.arrays().items():
        assert len(_check(src)) - 4 == want[k], k


@pytest.mark.parametrize("n", [0, 1, 12, 13, 14, 65535, 65536, 65537])
def test_edge_lengths(n):
    rng = np.random.default_rng(n)
    for src in (bytes(n), rng.integers(0, 256, n, dtype=np.uint8).tobytes(), rng.integers(0, 3, n, dtype=np.uint8).tobytes()):
        blob = _check(src)
        if n <= 12:   # all literals
            assert blob[4] >> 4 == min(n, 15) and blob[4] & 15 == 0
    assert R.dumps(b"") == b"\0\0\0\0\0"


def test_random_and_zeros():
    rng = np.random.default_rng(1)
    _check(rng.integers(0, 256, 100000, dtype=np.uint8).tobytes())
    blob = _check(bytes(300000))
    assert len(blob) - 4 == 1187


@pytest.mark.parametrize("k", [14, 15, 269, 270])
def test_literal_and_match_runs(k):
    """Literal runs and matches of exactly k bytes: the 15 / 255-byte continuation boundaries."""
    rng = np.random.default_rng(k)
    lit = rng.integers(1, 256, k - 1, dtype=np.uint8).tobytes()
    src = lit + bytes(41)                        # the first zero is a literal, the next one starts a match at offset 1
    seqs, _ = R.sequences(src)
    assert seqs[0][1] == k
    _check(src)
    head = rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
    rep = (head * ((k + 64) // 32 + 1))
    src = head + rep[32: 32 + k] + b"\x01" + rng.integers(0, 256, 20, dtype=np.uint8).tobytes()   # a match of exactly k at offset 32
    seqs, _ = R.sequences(src)
    assert any(L == k and off == 32 for _, _, off, L in seqs), seqs
    _check(src)


def test_offset_65535():
    rng = np.random.default_rng(2)
    a = np.zeros(70000, np.uint8)               # zeros between the two copies: no other position shares the pattern's hash
    a[100:120] = rng.integers(1, 256, 20, dtype=np.uint8)
    a[65535 + 100: 65535 + 120] = a[100:120]
    seqs, _ = R.sequences(a.tobytes())
    assert any(off == 65535 for _, _, off, _ in seqs)
    _check(a.tobytes())


def test_decoder_reads_liblz4_fixture():
    """tests/golden/lz4_foreign.npz (liblz4's own parse) decodes with the plain-Python decoder."""
    import gen_golden_lz4
    z = np.load(os.path.join(HERE, "golden", "lz4_foreign.npz"))
    for k, src in gen_golden_lz4.arrays().items():
        assert R.loads(z[k].tobytes()) == src, k


def test_decoder_rejects_malformed():
    blob = R.dumps(bytes(range(256)) * 8)
    for bad in (blob[:len(blob) // 2], blob[:3], struct.pack("<I", 8) + bytes([0x10, 0x41, 0, 0, 0x30]) + b"abc",
                struct.pack("<I", 2048 + 1) + blob[4:], struct.pack("<I", 2048 - 1) + blob[4:]):
        with pytest.raises(ValueError):
            R.loads(bad)
