"""Inputs of the deflate tests (tests/test_deflate_ref.py on the CPU, tests/test_gpu_deflate.py on the GPU) and their reference
streams, computed once per process."""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import deflate_ref as D  # noqa: E402

PINNED = {"contour_map": 4711, "idx_sequence": 2194, "plane_param": 536, "q_uniform": 47553, "q_nonuniform": 39777, "zeros": 326}


@functools.lru_cache(maxsize=None)
def golden_arrays():
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import gen_golden_lz4
    return gen_golden_lz4.arrays()


def far_pattern(distance, length=20):
    """40000 bytes, zero but for one pattern of `length` bytes and its copy `distance` bytes later."""
    rng = np.random.default_rng(5)
    a = np.zeros(40000, np.uint8)
    a[100:100 + length] = rng.integers(1, 256, length, dtype=np.uint8)
    a[distance + 100: distance + 100 + length] = a[100:100 + length]
    return a.tobytes()


@functools.lru_cache(maxsize=None)
def edge_inputs():
    """The smallest shapes at which each part of the encoder can go wrong."""
    rng = np.random.default_rng(7)
    out = {"len%d" % n: rng.integers(0, 4, n, dtype=np.uint8).tobytes() for n in (0, 1, 2, 3, 11, 12, 13, 14)}   # stored; the first matches
    out.update({"tile%d" % n: rng.integers(0, 4, n, dtype=np.uint8).tobytes() for n in (1034, 1035, 1036)})        # m = n - 11 around one tile
    out["two_letters"] = rng.integers(0, 2, 3000, dtype=np.uint8).tobytes()                                        # matches across tiles
    out.update({"zeros%d" % n: bytes(n) for n in (263, 264, 265, 266, 267, 268, 522, 523, 524, 525, 526, 781, 782)})   # the split rule
    out["offset_32768"] = far_pattern(32768)
    out["offset_32769"] = far_pattern(32769)
    out["random_65535"] = rng.integers(0, 256, 65535, dtype=np.uint8).tobytes()      # one stored block
    out["random_65536"] = rng.integers(0, 256, 65536, dtype=np.uint8).tobytes()      # two
    out["random_70000"] = rng.integers(0, 256, 70000, dtype=np.uint8).tobytes()
    fib = [1, 1]
    while len(fib) < 24:
        fib.append(fib[-1] + fib[-2])
    out["fibonacci"] = rng.permutation(np.repeat(np.arange(24, dtype=np.uint8), fib)).tobytes()   # 121392 bytes: the 15-bit limit
    lit = rng.integers(0, 64, 2500, dtype=np.uint8).tobytes()
    out["long_literals"] = lit + lit[:500]                                             # one sequence of ~2500 literals
    out["exact_fit"] = exact_fit()
    return out


def exact_fit():
    """100 bytes whose dynamic block is a whole number of bytes and exactly as large as the stored form (105): it is still the
    dynamic block, and the member fills bound(100) to the last byte."""
    for seed in range(10000):
        rng = np.random.default_rng(seed)
        src = rng.integers(0, 73, 100, dtype=np.uint8).tobytes()
        if D.dynamic_block(src)[1] == 8 * 105:
            return src
    raise AssertionError("no such input")


@functools.lru_cache(maxsize=None)
def reference(name):
    """deflate_ref.compress of a golden or edge input."""
    src = golden_arrays().get(name)
    return D.compress(edge_inputs()[name] if src is None else src)
