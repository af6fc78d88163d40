"""tests/bzip2_ref.py, the Python statement of the bzip2 encoder: every stream of tests/bzip2_cases.py is read by
bz2.decompress and by tests/bunzip2_ref.py, stays within the stated bound, is close to bz2.compress's size and is pinned by length and
sha256 in tests/golden/bzip2_pins.json; the cases land where their names say.  No GPU needed."""
import bz2
import functools
import hashlib
import json
import os

import pytest

import bunzip2_ref as D
import bzip2_cases as C
import bzip2_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = C.everything()


@functools.lru_cache(maxsize=None)
def stream(name):
    x, level = CASES[name]
    return R.compress(x, level)


@functools.lru_cache(maxsize=None)
def info(name):
    x, level = CASES[name]
    return R.stats(x, level)


@pytest.mark.parametrize("name", list(CASES))
def test_stream_decodes_and_is_pinned(name):
    x, level = CASES[name]
    s = stream(name)
    assert s[:4] == b"BZh" + bytes([0x30 + level])
    assert bz2.decompress(s) == x
    st, out, size, used = D.bunzip2(s, cap=len(x), nblock_max=100000 * level)
    assert (st, out, size, used) == (D.OK, x, len(x), len(s))
    assert len(s) <= R.bound(len(x), level)
    pin = json.load(open(os.path.join(HERE, "golden", "bzip2_pins.json")))[name]
    assert pin == {"input": len(x), "level": level, "length": len(s), "sha256": hashlib.sha256(s).hexdigest()}


def test_pins_cover_the_cases():
    assert sorted(json.load(open(os.path.join(HERE, "golden", "bzip2_pins.json")))) == sorted(CASES)


def test_sizes_against_libbz2():
    """On the four golden streams the total is not above bz2.compress's; every case of 1000 bytes or more is at most 0.5 % longer."""
    golden = [k for k in CASES if k.startswith("golden_")]
    assert len(golden) == 4
    assert sum(len(stream(k)) for k in golden) <= sum(len(bz2.compress(CASES[k][0])) for k in golden)
    assert [len(stream("golden_" + k)) for k in ("contour_map", "idx_sequence", "plane_param", "residual_quantized")] == [4732, 1815, 562, 29123]
    worst = 0.0
    for k, (x, level) in CASES.items():
        if len(x) >= 1000:
            ratio = len(stream(k)) / len(bz2.compress(x, level))
            print("%-24s %8d bytes  ratio %.5f" % (k, len(x), ratio))
            worst = max(worst, ratio)
            assert ratio <= 1.005, (k, ratio)
    print("worst ratio %.5f" % worst)


def test_empty_and_block_cut():
    assert stream("empty") == bz2.compress(b"") and len(stream("empty")) == 14
    assert [len(info(k)) for k in C.multi_block()] == [3, 2, 2, 1]
    assert info("below_limit")[0]["nblock"] == R.block_limit(1)
    # a run across the limit is cut between two of its sub-runs; the 4-into-5 expansion is what crosses the limit
    assert sum(b["nblock"] for b in info("run_across")) > R.block_limit(1) >= info("run_across")[0]["nblock"] > R.block_limit(1) - 5
    assert len(C.multi_block()["expansion"][0]) < R.block_limit(1) < sum(b["nblock"] for b in info("expansion"))
    for k in C.multi_block():
        assert all(b["nblock"] <= R.block_limit(1) for b in info(k)), k


def test_cases_land_where_their_names_say():
    for k, (seed, n, alpha) in C.NMTF.items():
        (b,) = info("nmtf%d" % k)
        assert b["nmtf"] == k and b["tables"] == R.table_count(k) and b["groups"] == -(-k // R.GROUP), (k, b)
    assert {R.table_count(k) for k in C.NMTF} == {2, 3, 4, 5, 6}
    assert {k % R.GROUP for k in C.NMTF} >= {49, 0, 1}
    (z,) = info("zero_runs")
    assert set(range(1, 41)) <= set(z["zruns"])
    assert info("zero_run_at_end")[0]["zruns"][-1] > 0 and info("ab300")[0]["zruns"][-1] > 0
    assert info("fibonacci")[0]["repairs"] > 0 and info("fibonacci")[0]["nblock"] > C.MTF_CHUNK * C.TILE
    assert info("all256")[0]["alpha"] == 258
    assert info("period1000")[0]["h"] >= 1024 and info("period1000")[0]["rounds"] >= 10
    for k in ("ab300", "abc1000", "period256x5", "period1000_whole"):     # equal rotations: doubling runs to h >= n
        assert info(k)[0]["h"] >= info(k)[0]["nblock"], k
    assert [info("golden_" + k)[0]["h"] for k in ("contour_map", "idx_sequence", "plane_param", "residual_quantized")] == [32, 512, 8, 256]


def test_code_lengths_rule():
    """The two-queue merge and the repair on counts small enough to follow by hand."""
    assert R.code_lengths([1, 1, 1], 17) == [2, 2, 1]
    assert R.code_lengths([5, 1, 1, 1], 17) == [1, 3, 3, 2]
    fib = [1, 1, 2, 3, 5, 8, 13, 21]
    assert R.code_lengths(fib, 17) == [7, 7, 6, 5, 4, 3, 2, 1]
    rep = [0]
    lens = R.code_lengths(fib, 4, rep)
    assert max(lens) == 4 and sum(2 ** (4 - l) for l in lens) == 16 and rep[0] > 0
    assert lens == sorted(lens, reverse=True)           # the longest lengths to the least frequent symbols
