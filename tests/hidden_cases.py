"""Named, seeded inputs of the hidden_points tests, shared by the CPU and the GPU files.  CASES[name]() -> one batch
dict(g=oracle.LidarGeom, frames=[f32 [N,4] rows, ...] (B = 3, the middle one empty), pad=(rows before offsets[0], rows behind
offsets[B]) or None); expected values come from tests/hidden_ref.py.

small / round2: the scenes of tests/subpixel_cases.py (three points per pixel on average: pixels with 0, 1 and several hidden points; two
rows of equal depth bits in one pixel; a nearer row in front of a depth-0 row, which is hidden though nearer than the owner; a pixel
emptied by a last depth-0 row, whose rows are uncarried; NaN / inf rows; clamped rows; the row that rounds to column W) with the edge rows
of edge_rows() behind them: rows on the y axis, whose fp32 depth is exactly the y they were given, at (k + 0.5) * step for even and odd k
(ties to even), at k * step, three times the same row (equal keys), and around k = 65535.
crowd: 3 000 rows in one pixel of SMALL (past the 255 cap, a segment longer than a workgroup), and pixels of 255, 256 and 257 rows
(254, 255 and 256 hidden points: below, at and past the cap) in the same frame; depths drawn from a few hundred values, so keys repeat.
past_the_grid: the batch of tests/intensity_cases.py sized past the cap of the row passes (tests/hidden_grid_caps.py)."""
import numpy as np

import intensity_cases as IC
import subpixel_cases as SC
from oracle import oracle as orc

STEP_POW2 = 2.0 ** -5          # d / step and k * step are exact: the tie rows are ties
STEP_TOOL = 0.04               # --accuracy 0.02
offsets = IC.offsets


def edge_rows(step):
    """Rows (0, d, 0, 0): depth exactly d.  -> (rows f32 [n,4], dict(name -> index)).  The first one is the nearest: it owns the pixel."""
    s = float(np.float32(step))
    f = np.float32
    d = dict(owner=0.25, tie_even=(10 + 0.5) * s, tie_odd=(11 + 0.5) * s, on_code=37 * s, below_tie=float(np.nextafter(f((20 + 0.5) * s), f(0))),
             above_tie=float(np.nextafter(f((20 + 0.5) * s), f(1e9))), same_a=123.25 * s, same_b=123.25 * s, same_c=123.25 * s,
             last=65535 * s, last_tie_below=float(np.nextafter(f(65535.5 * s), f(0))), last_tie=65535.5 * s, first_out=65536 * s, far_out=3.0e5 * s)
    rows = np.zeros((len(d), 4), np.float32)
    rows[:, 1] = np.array(list(d.values()), np.float32)
    return rows, {k: i for i, k in enumerate(d)}


def _scene(geom, seed, step):
    batch = SC._scene(orc.LidarGeom(**geom), seed)
    edge, where = edge_rows(step)
    f0, f1, f2 = batch["frames"]
    frames = [np.ascontiguousarray(np.concatenate([f0, edge])), f1, np.ascontiguousarray(np.concatenate([edge[::-1], f2]))]   # (reversed: the owner comes last)
    return dict(g=batch["g"], frames=frames, pad=batch["pad"], edge=where, step=step)


def small(step=STEP_POW2):
    return _scene(SC.SMALL, 1, step)


def round2(step=STEP_POW2):
    return _scene(SC.ROUND2, 2, step)


CROWD_AT = ((1, 5, 3000), (2, 9, 255), (2, 10, 256), (3, 17, 257))      # (row, column, rows aimed at the pixel)


def crowd():
    """B = 3: [the crowds among a cloud, empty, a cloud]."""
    g, rng = orc.LidarGeom(**SC.SMALL), np.random.default_rng(31)
    depths = np.round(rng.uniform(1.0, 60.0, 400), 2)                    # a few hundred values: equal depths, equal keys
    free = np.array([c for c in range(g.W) if c not in {col for _, col, _ in CROWD_AT}])
    parts = [IC.cloud(g, 150, rng, cols=free)]                             # (no cloud row in a crowd's column: the crowds' sizes are exact)
    for row, col, n in CROWD_AT:
        parts.append(IC.rays(g, row + rng.uniform(-0.3, 0.3, n), col + rng.uniform(-0.3, 0.3, n), rng.choice(depths, n), 0.0))
    f0 = np.concatenate(parts)
    f0 = f0[rng.permutation(f0.shape[0])]
    frames = [np.ascontiguousarray(f, dtype=np.float32) for f in (f0, np.zeros((0, 4), np.float32), IC.cloud(g, 200, rng))]
    return dict(g=g, frames=frames, pad=None, step=STEP_TOOL)


def example():
    return dict(SC.example(), step=STEP_TOOL)


def past_the_grid():
    """The cycle of tests/intensity_cases.py (seam, plain, zero, empty frames of 6001 / 6001 / 6001 / 0 rows at 16 x 512) until the batch holds
    more rows than one trip of the row passes takes."""
    import hidden_grid_caps as GC
    batch = IC.past_the_grid_frames(GC.HID_ROW_CAP * GC.HID_THREADS + 1, 0)
    return dict(g=batch["g"], frames=batch["frames"], pad=None, step=STEP_TOOL, distinct=batch["distinct"], which=batch["which"])


CASES = dict(small=small, round2=round2, crowd=crowd, example=example, past_the_grid=past_the_grid)
