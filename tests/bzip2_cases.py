"""Inputs of the bzip2 encoder's tests (tests/bzip2_ref.py, csrc_bzip2/bzip2_core.h, librpcc_bzip2.so), at the smallest sizes where a
stage can go wrong.  inputs(): name -> (bytes, level), built once.  The sizes named after the kernel are those of bzip2_core.h: tiles of
1024 keys, move-to-front chunks of 256 bytes, 4096 symbols per step of the emit stage."""
import bz2
import functools

import numpy as np

import bunzip2_cases

TILE, MTF_CHUNK, EMIT_STEP = 1024, 256, 4096

# (seed, length, alphabet) of random inputs found with the reference to give exactly this many symbols (nMTF): the thresholds of the
# number of tables (200 / 600 / 1200 / 2400) and group counts at a multiple of 50 and one beside it.  tests/test_bzip2_ref.py checks them.
NMTF = {
    199: (100, 198, 16),
    200: (100, 199, 16),
    599: (100, 598, 16),
    600: (100, 599, 16),
    1199: (100, 1201, 16),
    1200: (100, 1202, 16),
    2399: (106, 2401, 16),
    2400: (106, 2402, 16),
    249: (100, 248, 16),
    250: (100, 249, 16),
    251: (100, 250, 16),
}


def rnd(seed, n, alpha=256):
    return np.random.default_rng(seed).integers(0, alpha, n, dtype=np.uint8).tobytes()


def fibonacci(k=21, seed=9):
    """A block whose symbol counts force the 17-bit repair: k Fibonacci-skewed move-to-front ranks (rank r fib(k - r) times, shuffled)
    turned back into bytes p_i, each followed by the marker 255 and the binary digits of i.  The rotations that begin with the marker
    stand together in the order of i, so that stretch of the last column is p_1, p_2, ... and its ranks are the chosen ones; the digits
    add only to the counts of the first ranks, and no other byte value is used, so no count of 1 flattens the tree.  487152 bytes:
    also the one block of more than 1024 move-to-front chunks of 256 bytes."""
    f = [1, 1]
    while len(f) < k:
        f.append(f[-1] + f[-2])
    ranks = np.repeat(np.arange(k)[::-1], f)
    np.random.default_rng(seed).shuffle(ranks)
    order, p = list(range(k)), []
    for r in ranks.tolist():
        order.insert(0, order.pop(r))
        p.append(order[0])
    n = len(p)
    i, nd = np.arange(n), (n - 1).bit_length()
    out = np.empty((n, 2 + nd), np.uint8)
    out[:, 0], out[:, 1] = p, 255
    for d in range(nd):
        out[:, 2 + d] = (i >> (nd - 1 - d)) & 1
    return out.tobytes()


def zero_runs(top=41, seed=4):
    """For L = 1 .. top, L scattered copies of the pair (L, 100 + L), each followed by a random byte of 200 .. 255: the rotations that
    begin with 100 + L stand together, so the last column holds L times the byte L -- a zero run of L - 1 ranks."""
    rng = np.random.default_rng(seed)
    pairs = np.repeat(np.arange(1, top + 1), np.arange(1, top + 1))
    rng.shuffle(pairs)
    out = np.empty((pairs.size, 3), np.uint8)
    out[:, 0], out[:, 1], out[:, 2] = pairs, 100 + pairs, rng.integers(200, 256, pairs.size)
    return out.tobytes()


def golden_arrays():
    return {k: bz2.decompress(m) for k, m in bunzip2_cases.golden_members().items()}


@functools.lru_cache(maxsize=None)
def inputs():
    c = {"empty": (b"", 9), "one": (b"x", 9)}
    for r in (3, 4, 5, 255, 256, 259, 260, 1000):
        c["rep%d" % r] = (b"q" * r, 9)
    c["ab300"] = (b"ab" * 300, 9)
    c["abc1000"] = (b"abc" * 1000, 9)
    c["period256x5"] = (bytes(range(256)) * 5, 9)
    c["period7_runs"] = (b"aaaaabb" * 211, 9)
    c["all256"] = (bytes(range(256)), 9)
    c["all256_shuffled"] = (bytes(np.random.default_rng(2).permutation(256).astype(np.uint8)) * 3 + rnd(3, 500), 9)
    c["zero_runs"] = (zero_runs(), 9)
    c["zero_run_at_end"] = (b"ab" * 40 + b"b", 9)
    for k, (seed, n, alpha) in NMTF.items():
        c["nmtf%d" % k] = (rnd(seed, n, alpha), 9)
    c["fibonacci"] = (fibonacci(), 9)
    for n in (MTF_CHUNK - 1, MTF_CHUNK, MTF_CHUNK + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, EMIT_STEP - 1, EMIT_STEP, EMIT_STEP + 1,
              65535, 65536, 65537):
        c["len%d" % n] = (rnd(n, n, 3 if n % 2 else 200), 9)
    c["long_runs"] = (b"".join(bytes([v]) * r for v, r in zip(rnd(5, 60, 4), np.random.default_rng(6).integers(1, 3000, 60).tolist())), 9)
    pat = rnd(7, 1000)
    c["period1000"] = (pat * 65 + pat[:536], 9)                   # 64 KB: deep doubling
    c["period1000_whole"] = (pat * 8, 9)                          # equal rotations
    for k, v in golden_arrays().items():
        c["golden_" + k] = (v, 9)
    return c


@functools.lru_cache(maxsize=None)
def multi_block():
    """Level 1: inputs whose RLE1 bytes exceed one block of 99981."""
    c = {"blocks3": (rnd(12, 250000), 1)}
    c["run_across"] = (rnd(13, 99900, 7) + b"z" * 400 + rnd(14, 3000, 7), 1)
    c["expansion"] = (np.repeat(np.frombuffer(rnd(15, 22500), np.uint8), 4).tobytes(), 1)     # aaaabbbb...: 90000 bytes, 112500 and more after RLE1
    c["below_limit"] = (rnd(16, 99981), 1)                        # one block, full to the byte
    return c


def everything():
    return {**inputs(), **multi_block()}


# The many-thread host run (tests/test_bzip2_core_host.py) wakes 1024 threads at every barrier, a few milliseconds each time, so it takes
# the smallest input of each path -- nothing, one byte, runs at the RLE1 counts, a periodic block (equal rotations), a block whose
# bytes are all distinct (no doubling round), three tables, two move-to-front chunks, two tiles of keys -- and one input of two blocks
# at level 1: 100100 random bytes, no run of four among them, so the first block is full at 99981 and the second holds the other 119.
MANY_THREAD = ("empty", "one", "rep4", "rep5", "rep260", "ab300", "all256", "zero_run_at_end", "nmtf200", "len%d" % (MTF_CHUNK + 1), "len%d" % (TILE + 1))


@functools.lru_cache(maxsize=None)
def many_thread():
    c = {k: inputs()[k] for k in MANY_THREAD}
    c["two_blocks"] = (rnd(17, 100100), 1)
    return c
