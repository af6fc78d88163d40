"""Inputs of the row packer's tests (tests/rows_ref.py is the rule): the hostile table, seeded frames, and the frame patterns the GPU test
runs at every shape."""
import numpy as np

F = np.float32
INF, NAN = F(np.inf), F(np.nan)
DEN = F(1e-45)          # the smallest denormal
BIG = F(3e38)           # BIG + BIG overflows to inf

# (name, (x, y, z), kept): what (x + y) + z != 0 in fp32 decides
HOSTILE = [
    ("1e8 swallows 1, then cancels", (1e8, 1.0, -1e8), False),
    ("rotation: 1 - 1e8 rounds to -1e8", (1.0, -1e8, 1e8), False),
    ("rotation: the big ones cancel first", (-1e8, 1e8, 1.0), True),
    ("a real point the rule drops", (1.5, -1.5, 0.0), False),
    ("the same point, another order", (1.5, 0.0, -1.5), False),
    ("all zero", (0.0, 0.0, 0.0), False),
    ("-0.0 in x", (-0.0, 0.0, 0.0), False),
    ("-0.0 in y", (0.0, -0.0, 0.0), False),
    ("-0.0 in z", (0.0, 0.0, -0.0), False),
    ("-0.0 everywhere", (-0.0, -0.0, -0.0), False),
    ("denormals that cancel", (DEN, -DEN, 0.0), False),
    ("denormals that cancel late", (DEN, 0.0, -DEN), False),
    ("one denormal", (0.0, DEN, 0.0), True),
    ("two denormals", (DEN, DEN, 0.0), True),
    ("NaN in x", (NAN, 1.0, 2.0), True),
    ("NaN in y", (0.0, NAN, 0.0), True),
    ("NaN in z", (1.0, -1.0, NAN), True),
    ("inf - inf", (INF, -INF, 0.0), True),
    ("inf - inf late", (INF, 1.0, -INF), True),
    ("a finite sum that overflows", (BIG, BIG, 0.0), True),
    ("overflow, then -inf never comes", (BIG, BIG, -BIG), True),
    ("an ordinary point", (12.25, -3.5, 0.75), True),
]
# intensities that go with the table, cycled: NaN and -0.0 among them
HOSTILE_W = [0.25, NAN, -0.0, 0.0, 255.0, DEN, -1.0, INF]


def hostile_pc():
    return np.array([xyz for _, xyz, _ in HOSTILE], F)


def hostile_w():
    return np.array([HOSTILE_W[i % len(HOSTILE_W)] for i in range(len(HOSTILE))], F)


def hostile_kept():
    return np.array([k for _, _, k in HOSTILE], bool)


def seeded_frame(seed, P, empty=0.3):
    """A frame as a decoder leaves it: `empty` of the pixels all zero, the others points -> (pc [P,3], w [P], ri [P])."""
    rng = np.random.default_rng(seed)
    pc = rng.normal(0, 20, (P, 3)).astype(F)
    hole = rng.random(P) < empty
    pc[hole] = 0
    w = rng.random(P).astype(F)
    ri = np.where(hole, 0, np.sqrt((pc.astype(np.float64) ** 2).sum(-1))).astype(F)
    return pc, w, ri


PATTERNS = ("mixed", "all_kept", "none_kept", "empty_first", "empty_middle", "empty_last")


def batch(B, P, pattern, boundaries=(), seed=0):
    """pc [B,P,3], w [B,P], ri [B,P].  mixed: seeded frames with the hostile table laid across every boundary (pixel indices) that fits,
    at another phase in every frame; the empty_* patterns zero one frame of a mixed batch (its ri too)."""
    assert pattern in PATTERNS
    pcs, ws, ris = zip(*(seeded_frame(1000 * seed + 17 * B + b, P) for b in range(B)))
    pc, w, ri = np.stack(pcs), np.stack(ws), np.stack(ris)
    if pattern == "all_kept":
        pc = np.abs(pc) + F(1)
        ri = ri + F(1)
    elif pattern == "none_kept":
        pc[:] = 0
        pc[:, ::3] = (1.5, -1.5, 0.0)       # not empty, and still dropped
        ri[:, 1::2] = 0
    else:
        n = len(HOSTILE)
        for b in range(B):
            for at in (0,) + tuple(boundaries):
                lo = max(0, at - n // 2 - b)
                if lo + n <= P:
                    pc[b, lo: lo + n], w[b, lo: lo + n] = hostile_pc(), hostile_w()
        z = {"empty_first": 0, "empty_middle": B // 2, "empty_last": B - 1}.get(pattern)
        if z is not None:
            pc[z], ri[z] = 0, 0
    return np.ascontiguousarray(pc), np.ascontiguousarray(w), np.ascontiguousarray(ri)
