"""tests/rans_filter_ref.py, the Python statement of version 2 of the 'rans' format (the delta filter), against itself:
round trips at every width, version 1's bytes without the filter, the value and shape edges, the reset at every chunk's first element,
the 'RB' header rules, the size the filter buys on the example sweep's residuals, and the pins.  No GPU needed."""
import hashlib
import json
import os
import struct

import numpy as np
import pytest

import rans_cases as C1
import rans_filter_cases as C
import rans_filter_ref as F
import rans_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))


def test_every_case_round_trips_and_filter_0_is_version_1():
    forms = set()
    for name, (d, w, c, f) in C.valid().items():
        s = C.reference(name)
        assert F.decode(s, cap=len(d)) == (R.OK, d), name
        assert len(s) <= R.bound(len(d)), name
        forms.add((s[:2], s[2]))
        if f == F.FILTER_NONE:
            assert s == R.encode(d, w, c), name
        else:
            assert F.encode(d, w, c, F.FILTER_NONE) == R.encode(d, w, c), name
            assert s[:2] == b"RB" and s[9] == 1 or s == R.header(0, w, len(d), c) + d, name       # coded 'RB' or the version-1 stored stream
    assert forms == {(b"RA", 0), (b"RA", 1), (b"RB", 1)}
    for name, (s, d) in C.forced().items():
        assert s[:2] == b"RB" and F.decode(s) == (R.OK, d), name
    for name in C1.valid():                                  # version 1's own cases are read as before
        d = C1.valid()[name][0]
        assert F.decode(C1.reference(name)) == R.decode(C1.reference(name)) == (R.OK, d), name


@pytest.mark.parametrize("width", [1, 2, 4])
def test_filter_and_inverse(width):
    rng = np.random.default_rng(width)
    for clog in (8, 9, 16):
        for n in (0, 1, width - 1, width, width + 1, 255, 256 + width + 1, 3 * 256 + width - 1, 2000):
            d = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
            z = F.forward(d, width, clog)
            assert len(z) == n and F.inverse(z, width, clog) == d, (clog, n)
            assert z[n - n % width:] == d[n - n % width:]            # the cut element passes through
            per = (1 << clog) // width
            for e in range(0, n // width, per):                      # a chunk's first element is the zigzag of the value itself
                u = int.from_bytes(d[e * width: (e + 1) * width], "little")
                top = 1 << (8 * width - 1)
                want = (u << 1) if u < top else (((1 << 8 * width) - u) << 1) - 1
                assert int.from_bytes(z[e * width: (e + 1) * width], "little") == want, (clog, n, e)


def test_value_edges():
    alt = np.where(np.arange(700) % 2 == 0, -32768, 32767).astype("<i2").tobytes()
    z = np.frombuffer(F.forward(alt, 2, 9), "<u2")
    assert z[0] == 0xFFFF and z[256] == 0xFFFF                       # -32768 behind 0: d = 0x8000, z = 0xFFFF; again at the chunk's start
    assert set(z[1:256].tolist()) == {1, 2}                          # +65535 = -1 (z = 1) and -65535 = +1 (z = 2) modulo 2^16
    half = np.where(np.arange(300) % 2 == 0, 0, 0x80000000).astype("<u4").tobytes()
    z = np.frombuffer(F.forward(half, 4, 9), "<u4")
    assert z[0] == 0 and set(z[1:128].tolist()) == {0xFFFFFFFF} and z[128] == 0
    ramp = (np.arange(600) * 3 + 7).astype("<u2").tobytes()
    z = np.frombuffer(F.forward(ramp, 2, 9), "<u2")
    assert z[0] == 14 and z[256] == 2 * (256 * 3 + 7) and z[512] == 2 * (512 * 3 + 7) and set(np.delete(z, [0, 256, 512]).tolist()) == {6}
    zeros = F.encode(bytes(4096), 2, 9, F.FILTER_DELTA)
    assert zeros[:2] == b"RB" and zeros[12:17] == struct.pack("<HBH", 1, 0, 4095)       # one symbol, frequency 4096
    for d, w in ((alt, 2), (half, 4), (ramp, 2)):
        s = F.encode(d, w, 9, F.FILTER_DELTA)
        assert s[:2] == b"RB" and F.decode(s) == (R.OK, d)


def test_header_rules():
    s, data = C.base()
    assert s[:12] == b"RB" + bytes([1, 2]) + struct.pack("<I", len(data)) + bytes([9, 1, 0, 0])
    assert F.encode(b"", 2, 9, F.FILTER_DELTA) == F.encode(b"", 2, 9, F.FILTER_DELTA, fallback=False) == R.header(0, 2, 0, 9)
    codes = {}
    for name, (h, cap) in C.hostile().items():
        st, out = F.decode(h, cap)
        assert st != R.OK and out == b"", name
        assert F.parse(h, cap)[0] in (st, R.OK), name               # what the chunks find comes after the validation
        codes[name] = st
    assert all(codes["flip_header_%d" % k] == R.E_HEADER for k in list(range(32)) + list(range(72, 96)))     # magic, mode, width; filter, zeros
    assert {codes["flip_header_%d" % k] for k in range(32, 72)} <= {R.E_HEADER, R.E_CAPACITY, R.E_TABLE, R.E_TRUNCATED, R.E_DIRECTORY, R.E_STATE, R.E_PAYLOAD}
    for k in ("filter_0", "filter_2", "filter_255", "mode_0", "mode_0_stored_length", "reserved_10", "reserved_11", "n_0", "version_1_magic"):
        assert codes[k] == R.E_HEADER, k
    assert codes["cut_0"] == codes["cut_11"] == R.E_TRUNCATED and codes["n_above_capacity"] == R.E_CAPACITY
    assert codes["appended"] == R.E_DIRECTORY and codes["cut_%d" % (len(s) - 1)] == R.E_DIRECTORY


def test_the_filter_shrinks_the_example_residuals():
    """The size fact of DESIGN.md section 19: q_uniform of the example sweep (94 053 int16) at the default chunk size codes to 86 621
    bytes without the filter and to 30 222 with it."""
    q = np.load(os.path.join(HERE, "golden", "example_64E.npz"))["q_uniform"]
    assert q.dtype == np.int16 and q.size == 94053
    d = q.astype("<i2").tobytes()
    plain, filtered = R.encode(d, 2), F.encode(d, 2, filter=F.FILTER_DELTA)
    print("unfiltered %d bytes, filtered %d bytes: %.4f" % (len(plain), len(filtered), len(filtered) / len(plain)))
    assert filtered[:2] == b"RB" and F.decode(filtered) == (R.OK, d)
    assert len(filtered) <= 0.36 * len(plain)
    assert (len(plain), len(filtered)) == (86621, 30222)


def test_pins():
    pins = json.load(open(os.path.join(HERE, "golden", "rans_filter_pins.json")))
    assert len(pins) >= 10
    for name, pin in pins.items():
        if name == "golden_residual_quantized":
            d = np.load(os.path.join(HERE, "golden", "example_64E.npz"))["q_uniform"].astype("<i2").tobytes()
            s = F.encode(d, 2, filter=F.FILTER_DELTA)
        else:
            s = C.reference(name)
        assert (len(s), hashlib.sha256(s).hexdigest()) == (pin["length"], pin["sha256"]), name
