"""Inputs of the cloud packer's tests (tests/cloud_ref.py is the rule): the pixel segment comes from tests/rows_cases.py; these are the
extra segments and their counts."""
import numpy as np

import rows_cases as RC

F = np.float32
EXTRA_PATTERNS = ("mixed", "all_kept", "none_kept")
POISON = F(777.0)       # what lies behind a frame's count: kept by the rule, so reading it shows


def extras(B, capacity, pattern, counts, boundaries=(), seed=0):
    """extra f32 [B,capacity,3]: frame b's first clamp(counts[b]) points follow `pattern` -- mixed: seeded points, a third of them (0, 0, 0),
    with the hostile table of rows_cases laid across every boundary (point indices) that fits, at another phase in every frame --; every
    point behind them is POISON."""
    assert pattern in EXTRA_PATTERNS
    out = np.full((B, capacity, 3), POISON, F)
    n_h = len(RC.HOSTILE)
    for b in range(B):
        n = min(max(int(counts[b]), 0), capacity)
        pts = RC.seeded_frame(5000 + 1000 * seed + 31 * B + b, n)[0] if n else np.zeros((0, 3), F)
        if pattern == "all_kept":
            pts = np.abs(pts) + F(1)
        elif pattern == "none_kept":
            pts[:] = 0
            pts[::3] = (1.5, -1.5, 0.0)        # not empty, and still dropped
        else:
            for at in (0,) + tuple(boundaries):
                lo = max(0, at - n_h // 2 - b)
                if lo + n_h <= n:
                    pts[lo: lo + n_h] = RC.hostile_pc()
        out[b, :n] = pts
    return np.ascontiguousarray(out)


def counts_for(B, capacity, kind):
    """The per-frame counts of a batch: `kind` (a name, or a count) for frame 0, then a cycle through the other kinds, so that every batch of B > 1 mixes them."""
    table = dict(zero=0, one=1, full=capacity, above=capacity + 5, negative=-3, half=capacity // 2)
    order = [kind] + [k for k in ("full", "zero", "above", "one", "negative", "half") if k != kind]
    return np.array([table.get(order[b % len(order)], order[b % len(order)]) for b in range(B)], np.int32)      # (an int: that count itself)
