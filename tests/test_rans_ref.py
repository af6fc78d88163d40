"""tests/rans_ref.py, the Python statement of the 'rans' format, on tests/rans_cases.py: it round-trips every valid
case, its normalisation holds the stated properties, every hostile stream is refused with no output, every coded chunk stays within the
bound a sound rANS coder obeys (derived below, independent of the code under test), and its streams equal tests/golden/rans_pins.json.
No GPU needed."""
import json
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import gen_rans_pins  # noqa: E402
import rans_cases as C  # noqa: E402
import rans_ref as R  # noqa: E402


def test_case_table_covers_what_it_names():
    v = C.valid()
    for n in C.LENGTHS:
        for w in C.WIDTHS:
            for content in ("one", "two", "dominant", "even", "random"):
                assert "%s_n%d_w%d" % (content, n, w) in v
        assert "int16_n%d_w2" % n in v and "float32_n%d_w4" % n in v
    ref = {k: C.reference(k) for k in C.everything()}
    assert all(ref[k][2] == 0 for k, (d, w, c) in v.items() if c == 8)                  # 256-byte chunks: the flush alone is as long
    # all 256 symbols evenly (at width 1: a wider stream's planes see every second or fourth symbol only) and random bytes: stored
    assert all(ref[k][2] == 0 for k in v if k.split("_")[1] == "random" or (k.split("_")[1] == "even" and k.endswith("_w1")))
    coded = [k for k in ref if ref[k][2] == 1]
    assert {k.split("_")[1] for k in coded if k.startswith("c1")} >= {"one", "two", "dominant", "int16", "float32"}
    assert any(k.startswith("default_") for k in coded) and sum(k.startswith("golden_") for k in coded) == 4
    assert len(ref["one_n0_w1"]) == 12


def test_round_trip_of_every_valid_case():
    for name, (d, w, c) in C.everything().items():
        s = C.reference(name)
        assert len(s) <= R.bound(len(d)), name
        assert R.decode(s, cap=len(d)) == (R.OK, d), name
    for name, (s, d) in C.forced().items():
        assert s[2] == 1 and R.decode(s, cap=len(d)) == (R.OK, d), name
    one = C.forced()["one_n515_w1"][0]                     # one symbol: frequency 4096, no words at all
    assert len(one) == 12 + 2 + 3 + 3 * 4 + 4 * (64 + 64 + 3)


def _check_normalised(counts, f):
    assert sum(f) == R.PROB
    assert all((c == 0) == (v == 0) for c, v in zip(counts, f))
    total, raw = sum(counts), None
    raw = [max(1, c * R.PROB // total) if c else 0 for c in counts]
    top = raw.index(max(raw))
    if sum(raw) <= R.PROB:                                 # the remainder goes to the largest, the lowest such symbol
        assert f == [v + (R.PROB - sum(raw) if s == top else 0) for s, v in enumerate(raw)]
    else:                                                  # the deficit comes off the largest: nobody gains, nobody falls below 1
        assert all(1 <= v <= r for v, r in zip(f, raw) if r)
        lowered = [s for s in range(256) if f[s] < raw[s]]
        assert all(f[s] >= max(f) - 1 for s in lowered)    # what was lowered ends level with the top


def test_normalisation_properties():
    deficits = 0
    for name, (d, w, c) in C.everything().items():
        for p in range(w):
            plane = d[p::w]
            if plane:
                counts = np.bincount(np.frombuffer(plane, np.uint8), minlength=256).tolist()
                f = R.normalise(counts)
                _check_normalised(counts, f)
                deficits += sum(max(1, c * R.PROB // len(plane)) for c in counts if c) > R.PROB
    assert deficits >= 3
    rng = np.random.default_rng(5)
    for trial in range(200):
        m = int(rng.integers(1, 257))
        counts = np.zeros(256, np.int64)
        counts[rng.permutation(256)[:m]] = np.maximum(1, (rng.pareto(0.7, m) * rng.integers(1, 50)).astype(np.int64))
        _check_normalised(counts.tolist(), R.normalise(counts.tolist()))
    assert R.normalise([0] * 7 + [5] + [0] * 248)[7] == R.PROB
    tie = R.normalise([3, 3, 3] + [0] * 253)               # 1365 each, remainder 1: to the lowest of the equal symbols
    assert tie[:3] == [1366, 1365, 1365]


def test_hostile_streams_are_refused_without_output():
    h = C.hostile()
    assert sum(k.startswith("flip_header") for k in h) == 96 and sum(k.startswith("flip_table") for k in h) == 8 * 770
    assert sum(k.startswith("flip_directory") for k in h) == 96 and sum(k.startswith("cut_") for k in h) == len(C.base()[0])
    for name, (s, cap) in h.items():
        st, out = R.decode(s, cap=cap)
        assert st != R.OK and out == b"", name
    st = lambda k: R.decode(*h[k])[0]
    assert st("payload_word_flipped") == R.E_STATE
    assert st("n_above_capacity") == R.E_CAPACITY and st("appended") == R.E_DIRECTORY and st("freq_sum_changed") == R.E_TABLE
    assert st("directory_exchanged") == R.E_PAYLOAD and st("freq_sum_kept") < 0
    assert {R.decode(*h[k])[0] for k in h if k.startswith("cut_")} == {R.E_TRUNCATED, R.E_DIRECTORY}


def test_every_coded_chunk_obeys_the_rans_bound():
    """With f the frequencies stored in the stream and k the chunk's bytes, a payload is at most 4 min(64, k) + (sum log2(4096 / f[s]) +
    0.0875 k) / 8 + 1 bytes: one coding step maps x to less than x 4096 / f + 4096, and the state before it is at least 16 f after
    renormalisation, so a step adds at most log2(4096 / f) + log2(17 / 16) < log2(4096 / f) + 0.0875 bits to log2 x; each word emitted
    takes at least 16 bits off, and the flush is 32 bits per lane."""
    streams = [(k, C.reference(k), C.everything()[k][0]) for k in C.everything()] + [(k, s, d) for k, (s, d) in C.forced().items()]
    checked = 0
    for name, s, d in streams:
        if s[2] != 1:
            continue
        st, (mode, width, n, clog, freqs, spans) = R.parse(s, len(d))
        assert st == R.OK
        cost = [[math.log2(R.PROB / f) if f else None for f in fr] for fr in freqs]
        for c, (_, plen) in enumerate(spans):
            chunk = d[c << clog: (c + 1) << clog]
            bits = sum(cost[(i % 64) % width][b] for i, b in enumerate(chunk))
            assert plen <= 4 * min(64, len(chunk)) + (bits + 0.0875 * len(chunk)) / 8 + 1, (name, c)
            checked += 1
    assert checked > 500


def test_reference_streams_equal_their_pins():
    pins = json.load(open(os.path.join(HERE, "golden", "rans_pins.json")))
    assert gen_rans_pins.pins() == pins
