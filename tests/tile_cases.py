"""Generators of the cases that take the eval and DBSCAN searches past one round of the tile list, past one chunk of the
row scan, through partial tiles and onto the edges of their comparisons (numpy only).  Every generator returns its inputs and
a dict of the facts it claims about itself; tests/test_tile_cases.py asserts those facts on the CPU, so a case cannot
silently stop exercising what it is for, and tests/test_gpu_tile_search.py runs the cases on the device.

DBSCAN inputs are (ri f32 [H,W], tm f32 [H,W,3], ground f64 [4]) with the conventions of dbscan_ref.frame: the plane is
dbscan_ref.GROUND = (0, 0, 1, 1); a real point p is the pixel ri = 1, tm = p (non-ground when |1 + 1/p.z| > 0.5: p.z is 0 or
lies in [0.1, 10]); a ground pixel is ri = 1, tm = (0, 0, -1); a zero-range pixel is ri = 0, tm = (1, 0, 0).
Eval inputs are (p1, p2 f32 [H,W,3]); a pixel without a point is (0, 0, 0)."""
import numpy as np

import dbscan_ref

F32 = np.float32
TILE_R, TILE_C, TILE_LIST = 8, 32, 1024   # csrc_tile/tiles.h
SCAN_CHUNK = 256                          # rows per step of scan_kernel
MAX_REAL = 40000                          # real points per frame: the numpy references stay cheap below it
GROUND = dbscan_ref.GROUND
SWEEP_EPS = (0.05, 0.45, 1.5, 6.0, 40.0)
SWEEP_MIN_POINTS = (1, 2, 10, 50)


# ------------------------------------------------------------------------------------------------
# tiles, as the libraries cut them
# ------------------------------------------------------------------------------------------------
def tile_count(H, W):
    return -(-H // TILE_R) * -(-W // TILE_C)


def tile_index(H, W):
    """int [H,W]: the tile of every pixel, tiles numbered row-major over the tile grid."""
    hh, ww = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return (hh // TILE_R) * -(-W // TILE_C) + ww // TILE_C


def tile_boxes(pts, valid):
    """(lo, hi f32 [T,3], count [T]) of the valid points of an [H,W,3] image per tile; empty tiles get lo = +inf, hi = -inf."""
    H, W = valid.shape
    T = tile_count(H, W)
    t = tile_index(H, W)[valid]
    p = np.asarray(pts, F32)[valid]
    lo, hi = np.full((T, 3), np.inf, F32), np.full((T, 3), -np.inf, F32)
    np.minimum.at(lo, t, p)
    np.maximum.at(hi, t, p)
    return lo, hi, np.bincount(t, minlength=T)


def box_bound(qlo, qhi, lo, hi):
    """tiles.h's box_bound in numpy float32: per axis ONE rounded subtraction of box faces, clamped at 0, then
    ((gx*gx) + (gy*gy)) + (gz*gz).  qlo, qhi [n,3] against lo, hi [m,3] -> f32 [n,m]."""
    g = np.maximum(np.maximum(lo[None] - qhi[:, None], qlo[:, None] - hi[None]), F32(0))
    g = g.astype(F32)
    return (g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2]


def screen_bounds(eps):
    """(lo, hi) of the fp32 screen of rpcc_seg_dbscan: eps^2 (1 -+ 8 * 2^-24), rounded inwards (lo down, hi up) to fp32."""
    e2 = float(eps) * float(eps)
    u8 = 8.0 * 2.0 ** -24
    lo64, hi64 = e2 * (1.0 - u8), e2 * (1.0 + u8)
    lo, hi = F32(lo64), F32(hi64)
    if float(lo) > lo64:
        lo = np.nextafter(lo, F32(0))
    if float(hi) < hi64:
        hi = np.nextafter(hi, F32(np.inf))
    return lo, hi


def d2f(p, q):
    """The kernels' fp32 distance (tiles.h dist3): ((dx*dx) + (dy*dy)) + (dz*dz), dx = p - q, every step rounded to fp32."""
    p, q = np.asarray(p, F32), np.asarray(q, F32)
    dx, dy, dz = p[..., 0] - q[..., 0], p[..., 1] - q[..., 1], p[..., 2] - q[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def d2_exact(p, q):
    """dbscan_ref.d2 on fp32 points widened to fp64."""
    return dbscan_ref.d2(np.asarray(p, F32).astype(np.float64), np.asarray(q, F32).astype(np.float64))


# ------------------------------------------------------------------------------------------------
# frames
# ------------------------------------------------------------------------------------------------
def ground_frame(H, W):
    ri = np.ones((H, W), F32)
    tm = np.zeros((H, W, 3), F32)
    tm[..., 2] = -1.0
    return ri, tm


def put_points(ri, tm, pix, pts):
    """Real points pts [n,3] on the flat pixels pix; asserts that each is non-ground by the convention above."""
    pts = np.asarray(pts, F32).reshape(-1, 3)
    z = pts[:, 2]
    assert np.all((z == 0) | ((z >= F32(0.1)) & (z <= 10))), "p.z must be 0 or in [0.1, 10]"
    ri.reshape(-1)[pix] = 1.0
    tm.reshape(-1, 3)[pix] = pts


def put_zero_range(ri, tm, pix):
    ri.reshape(-1)[pix] = 0.0
    tm.reshape(-1, 3)[pix] = (1.0, 0.0, 0.0)


def real_mask(ri, tm):
    """bool [H,W]: the pixels that hold a real (non-ground, non-zero-range) point."""
    return dbscan_ref.nonground(ri, tm, GROUND) & (np.asarray(ri) != 0)


def check_frame(ri, tm):
    n = int(real_mask(ri, tm).sum())
    assert n <= MAX_REAL, "%d real points: the numpy reference is not cheap any more" % n
    return n


def cut_high_tiles(ri, tm, first=TILE_LIST):
    """The frame with every pixel of a tile >= first turned into ground: what a search that stops after the first round of the
    tile list sees of it."""
    H, W = ri.shape
    ri2, tm2 = ri.copy(), tm.copy()
    cut = tile_index(H, W) >= first
    ri2[cut] = 1.0
    tm2[cut] = (0.0, 0.0, -1.0)
    return ri2, tm2


def second_frame(ri, tm, band=64, seed=1):
    """A second frame over the same tm (dbscan_segment takes one tm per call and tm holds the points): ri = 2 on every other
    band of `band` rows (or columns when the image is wider than high), which moves those points to 2p, and a few more
    pixels zeroed."""
    H, W = ri.shape
    hh, ww = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    along = hh if H >= W else ww
    ri2 = ri.copy()
    sel = ((along // band) % 2 == 1) & real_mask(ri, tm)
    pz = tm[..., 2]
    sel &= (pz == 0) | ((pz >= F32(0.1)) & (pz <= 5))     # 2p keeps the z convention
    ri2[sel] = 2.0
    rng = np.random.default_rng(seed)
    cand = np.nonzero(real_mask(ri, tm).reshape(-1))[0]
    ri2.reshape(-1)[rng.choice(cand, min(25, cand.size), replace=False)] = 0.0
    return ri2


def eval_valid(p):
    p = np.asarray(p, F32)
    return ((p[..., 0] + p[..., 1]) + p[..., 2]) != 0


def check_eval_cloud(p, real):
    """Every real pixel holds a point the metrics count ((x + y) + z != 0 in fp32), every other pixel none."""
    assert np.array_equal(eval_valid(p), real), "a real point with (x + y) + z == 0 is not a point to the metrics"


# ------------------------------------------------------------------------------------------------
# folded: two pixel-coherent sheets, the second in the far half of the image
# ------------------------------------------------------------------------------------------------
FOLDED_SHAPES = ((2048, 160), (72, 4096))
# (eps, min_points) per shape.  The first pair is the one measured when the case was designed (2048 x 160: sheet A alone gives
# 5 neighbours per point, A + B 6); the second has a larger eps and was chosen by the same assertion
# (test_tile_cases.test_folded_depends_on_second_round), not by hand: 2 819 labels of tiles < 1024 depend on the tiles >= 1024
# on 2048 x 160; on 72 x 4096 the pairs give 33 and 10 752 (at (0.9, 15) the bridge joins all the bands into one cluster).
FOLDED_PARAMS = {(2048, 160): ((0.45, 6), (0.9, 20)), (72, 4096): ((0.45, 6), (0.9, 15))}


def folded(H, W, spacing=0.4, gap=0.3, seed=9):
    """Sheet A: a lattice of real points on every 4th row and column of the first half of the image (z = 0, 0.01 m jitter in
    x and y).  Sheet B: the same lattice lifted by `gap` in the second half.  The image is folded along its longer side, so
    a point of A and the point of B above it are half an image apart.  Empty bands cut the sheets into several clusters;
    where the fold runs along the columns (the tile index then grows along the fold only inside a tile row) the bands stop
    short of the tiles >= TILE_LIST, which bridge the clusters there.  A sprinkle of zero-range pixels is added.
    -> (ri, tm, ground), facts."""
    rng = np.random.default_rng(seed)
    hh, ww = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    rows = H >= W                                   # fold along the rows
    along, across = (hh, ww) if rows else (ww, hh)
    half = (H if rows else W) // 2
    step = spacing / 4.0
    upper = along >= half
    base = np.stack([step * across, step * (along % half), np.where(upper, gap, 0.0)], -1)
    jit = rng.normal(0, 0.01, base.shape)
    jit[..., 2] = np.where(upper, jit[..., 2], 0.0)  # sheet A keeps z = 0 exactly
    p = (base + jit).astype(F32)
    real = (hh % 4 == 0) & (ww % 4 == 0)
    band = ((along % half) % (half // 8)) < 3 * (half // 32)
    tile = tile_index(H, W)
    real &= band if rows else (band | (tile >= TILE_LIST))
    ri, tm = ground_frame(H, W)
    put_points(ri, tm, np.nonzero(real.reshape(-1))[0], p[real])
    zero = (rng.random((H, W)) < 0.001) & ~real
    put_zero_range(ri, tm, np.nonzero(zero.reshape(-1))[0])
    n = check_frame(ri, tm)
    facts = dict(T=tile_count(H, W), real=n, zero=int(zero.sum()), rows=rows, half=half, params=FOLDED_PARAMS.get((H, W), ()))
    return (ri, tm, GROUND.copy()), facts


def folded_eval(H, W, spacing=0.4, gap=0.3, seed=9):
    """Eval variant of folded: cloud 1 holds the real points, cloud 2 is cloud 1 with part of it blanked, so that the nearest
    cloud-2 point of a blanked point lies half an image away (fold along the rows: the last quarter of sheet A is blanked and
    the answer is the point of B above it) or across the last tile row (fold along the columns: the two real rows below the
    last tile row are blanked in both sheets).  -> (p1, p2), facts; facts['blank'] is the blanked pixel mask."""
    (ri, tm, _), f = folded(H, W, spacing, gap, seed)
    real = real_mask(ri, tm)
    p1 = np.where(real[..., None], tm, F32(0)).astype(F32)
    hh, ww = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    if f["rows"]:
        blank = real & (hh >= f["half"] // 2) & (hh < f["half"])
    else:
        last = (H - 1) // TILE_R * TILE_R          # first row of the last tile row
        blank = real & (hh >= last - TILE_R) & (hh < last)
    p2 = p1.copy()
    p2[blank] = 0
    check_eval_cloud(p1, real)
    check_eval_cloud(p2, real & ~blank)
    return (p1, p2), dict(T=f["T"], n1=int(real.sum()), n2=int((real & ~blank).sum()), blank=blank)


def nn_crossings(p1, p2, idx12, first=TILE_LIST):
    """Number of cloud-1 points whose nearest cloud-2 point (idx12: ranks in cloud 2) lies on the other side of tile `first`."""
    H, W = p1.shape[:2]
    tile = tile_index(H, W).reshape(-1)
    t1 = tile[np.nonzero(eval_valid(p1).reshape(-1))[0]]
    t2 = tile[np.nonzero(eval_valid(p2).reshape(-1))[0]]
    return int(np.count_nonzero((t1 < first) != (t2[idx12] < first)))


# ------------------------------------------------------------------------------------------------
# scattered: a blob cloud thrown on random pixels, every tile's box spans the scene
# ------------------------------------------------------------------------------------------------
SCATTERED_SHAPES = ((2048, 160, 20000), (8, 32768, 12000), (8, 32769, 12000))
SCATTERED_PARAMS = ((1.5, 10), (0.45, 4))


def _blob_cloud(rng, n, blobs=60):
    c = rng.uniform(-40, 40, (blobs, 3))
    c[:, 2] = rng.uniform(2, 8, blobs)
    p = c[rng.integers(0, blobs, n)] + rng.normal(0, 0.8, (n, 3))
    m = n // 10                                     # 10 % uniform noise
    p[:m] = rng.uniform(-50, 50, (m, 3))
    p[:m, 2] = rng.uniform(0.1, 10, m)
    p[:, 2] = np.clip(p[:, 2], 0.1, 10)
    return p.astype(F32)


ANCHOR = (80.0, 80.0, 5.0)   # a point outside the scene (the blobs and the noise stay within 50 m of the origin per axis)
ANCHOR_COPIES = max(mp for _, mp in SCATTERED_PARAMS)


def _anchor_pixels(H, W):
    """The last pixel of the image, which lies in the last tile whatever its width, and ANCHOR_COPIES - 1 pixels of tile 0."""
    assert W >= ANCHOR_COPIES
    return np.array([H * W - 1] + list(range(ANCHOR_COPIES - 1)))


def scattered(H, W, n, seed=5, zero=200):
    """-> (ri, tm, ground), facts.  facts['T'] is the tile count; that the tile list fills is the claim scattered_fill checks.
    ANCHOR_COPIES copies of ANCHOR, one on the last pixel of the last tile and the others in tile 0, are core at the largest
    min_points of SCATTERED_PARAMS only if the search reaches the last tile (on 8 x 32769 a one-column tile that the random
    pixels may well leave empty)."""
    rng = np.random.default_rng(seed)
    n = min(n, H * W)
    anchor = _anchor_pixels(H, W)
    m = n - anchor.size
    zero = min(zero, H * W - n)
    p = _blob_cloud(rng, m)
    ri, tm = ground_frame(H, W)
    free = np.setdiff1d(np.arange(H * W), anchor)
    pix = free[rng.choice(free.size, m + zero, replace=False)]
    put_points(ri, tm, pix[:m], p)
    put_points(ri, tm, anchor, np.tile(ANCHOR, (anchor.size, 1)))
    put_zero_range(ri, tm, pix[m:])
    assert check_frame(ri, tm) == n
    return (ri, tm, GROUND.copy()), dict(T=tile_count(H, W), real=n, zero=zero, params=SCATTERED_PARAMS, anchor=anchor)


def scattered_fill(ri, tm, eps):
    """Fraction of the ordered pairs of non-empty tiles (t != t') with box_bound <= eps^2 (the list filter keeps a tile up to
    the screen's hi, which is above eps^2), and the number of non-empty tiles."""
    lo, hi, cnt = tile_boxes(tm, real_mask(ri, tm))
    k = np.nonzero(cnt)[0]
    e2 = F32(float(eps) * float(eps))
    kept = 0
    for c0 in range(0, k.size, 128):
        q = k[c0:c0 + 128]
        kept += int(np.count_nonzero(box_bound(lo[q], hi[q], lo[k], hi[k]) <= e2)) - q.size   # minus the tile itself
    return kept / max(k.size * (k.size - 1), 1), int(k.size)


def scattered_eval(H, W, n, seed=5):
    """Cloud 1: the blob cloud on random pixels; cloud 2: a 0.05 m jittered copy of nine tenths of it on other random pixels,
    so the co-located tile is no help and every tile of every round has to be considered.  Cloud 1 holds ANCHOR on pixel 0 and
    cloud 2 holds it on the last pixel of the last tile: the answer to that query lies in the last tile.  -> (p1, p2), facts."""
    rng = np.random.default_rng(seed + 100)
    n = min(n, H * W)
    a = _blob_cloud(rng, n - 1)
    m = max(1, (9 * n) // 10)
    b = (a[rng.permutation(n - 1)[:m - 1]] + rng.normal(0, 0.05, (m - 1, 3))).astype(F32)
    p1, p2 = np.zeros((H * W, 3), F32), np.zeros((H * W, 3), F32)
    k1 = 1 + rng.choice(H * W - 2, n - 1, replace=False)       # neither pixel 0 nor the last
    k2 = 1 + rng.choice(H * W - 2, m - 1, replace=False)
    p1[k1], p2[k2] = a, b
    p1[0], p2[H * W - 1] = ANCHOR, ANCHOR
    r1, r2 = np.zeros(H * W, bool), np.zeros(H * W, bool)
    r1[k1], r2[k2], r1[0], r2[H * W - 1] = True, True, True, True
    p1, p2 = p1.reshape(H, W, 3), p2.reshape(H, W, 3)
    check_eval_cloud(p1, r1.reshape(H, W))
    check_eval_cloud(p2, r2.reshape(H, W))
    return (p1, p2), dict(T=tile_count(H, W), n1=n, n2=m)


# ------------------------------------------------------------------------------------------------
# small shapes: partial row and column tiles, H > 256
# ------------------------------------------------------------------------------------------------
SMALL_SHAPES = ((1, 1), (1, 1031), (7, 33), (9, 31), (257, 40), (300, 64))
SMALL_PARAMS = ((1.5, 4), (0.45, 2))


def _small_cloud(rng, n):
    blobs = max(3, n // 150)                         # the scene grows with the cloud: the density stays what it is
    c = rng.uniform(-3, 3, (blobs, 3)) * blobs ** 0.5
    c[:, 2] = rng.uniform(2, 8, blobs)
    p = c[rng.integers(0, blobs, n)] + rng.normal(0, 0.5, (n, 3))
    p[:, 2] = np.clip(p[:, 2], 0.1, 10)
    return p.astype(F32)


def small_shapes(seed=21):
    """-> list of ((ri, tm, ground), (p1, p2), facts), one per shape of SMALL_SHAPES: a blob cloud on 60 % of the pixels, 5 %
    zero-range pixels; the eval pair is the cloud and a jittered, thinned copy on other pixels."""
    out = []
    for i, (H, W) in enumerate(SMALL_SHAPES):
        rng = np.random.default_rng(seed + i)
        P = H * W
        n = max(1, (6 * P) // 10)
        zero = P // 20
        p = _small_cloud(rng, n)
        ri, tm = ground_frame(H, W)
        pix = rng.choice(P, n + zero, replace=False)
        put_points(ri, tm, pix[:n], p)
        put_zero_range(ri, tm, pix[n:])
        assert check_frame(ri, tm) == n
        m = max(1, (8 * n) // 10)
        b = (p[rng.permutation(n)[:m]] + rng.normal(0, 0.05, (m, 3))).astype(F32)
        p1, p2 = np.zeros((P, 3), F32), np.zeros((P, 3), F32)
        p1[pix[:n]] = p
        k2 = rng.choice(P, m, replace=False)
        p2[k2] = b
        r1, r2 = np.zeros(P, bool), np.zeros(P, bool)
        r1[pix[:n]], r2[k2] = True, True
        p1, p2 = p1.reshape(H, W, 3), p2.reshape(H, W, 3)
        check_eval_cloud(p1, r1.reshape(H, W))
        check_eval_cloud(p2, r2.reshape(H, W))
        facts = dict(H=H, W=W, T=tile_count(H, W), real=n, zero=zero, n1=n, n2=m, params=SMALL_PARAMS,
                     partial_rows=H % TILE_R != 0, partial_cols=W % TILE_C != 0, second_scan_chunk=H > SCAN_CHUNK)
        out.append(((ri, tm, GROUND.copy()), (p1, p2), facts))
    return out


# ------------------------------------------------------------------------------------------------
# sweep: the random blobs of test_seg_abi.test_reference_against_sklearn_random over eps x min_points
# ------------------------------------------------------------------------------------------------
SWEEP_SEEDS = {0: (16, 128), 1: (16, 128), 2: (64, 512)}
SWEEP_REAL_64 = 2000   # real points kept on 64 x 512: at eps = 40 every pair is a neighbour pair, and the reference lists them


def sweep_cloud(seed):
    """-> (ri, tm, ground), facts.  Even seeds have about 10 % zero-range pixels (the origin point is core at every min_points of
    the sweep), odd seeds exactly three (it is not at min_points 10 and 50 and small eps).  On 64 x 512 all but SWEEP_REAL_64 of
    the real points are turned into ground."""
    H, W = SWEEP_SEEDS[seed]
    rng = np.random.default_rng(seed)
    n = H * W
    centres = rng.uniform(-20, 20, (12, 2))
    xy = centres[rng.integers(0, 12, n)] + rng.normal(0, rng.uniform(0.3, 1.5), (n, 2))
    tm = np.zeros((n, 3), F32)
    tm[:, :2] = xy
    ri = np.ones(n, F32)
    if seed % 2 == 0:
        ri[rng.random(n) < 0.1] = 0.0
    else:
        ri[rng.choice(n, 3, replace=False)] = 0.0
    tm[ri == 0] = (1.0, 0.0, 0.0)
    ground_pix = (rng.random(n) < 0.1) & (ri != 0)
    real = np.nonzero(~ground_pix & (ri != 0))[0]
    if real.size > SWEEP_REAL_64 and (H, W) == (64, 512):
        drop = rng.permutation(real)[SWEEP_REAL_64:]
        ground_pix[drop] = True
    tm[ground_pix] = (0.0, 0.0, -1.0)
    ri, tm = ri.reshape(H, W), tm.reshape(H, W, 3)
    nreal = check_frame(ri, tm)
    return (ri, tm, GROUND.copy()), dict(H=H, W=W, real=nreal, zero=int((ri == 0).sum()), eps=SWEEP_EPS, min_points=SWEEP_MIN_POINTS)


def has_exact_pair(ri, tm, eps):
    """Whether two real points, or a real point and the origin, sit at d^2 == eps^2 exactly in fp64 (dense: small frames only)."""
    p = dbscan_ref.points(ri, tm)[real_mask(ri, tm)].astype(np.float64)
    assert p.shape[0] <= 12000
    e2 = float(eps) * float(eps)
    if np.any(dbscan_ref.d2(p, np.zeros(3)) == e2):
        return True
    for c0 in range(0, p.shape[0], 512):
        if np.any(dbscan_ref.d2(p[c0:c0 + 512, None], p[None]) == e2):
            return True
    return False


# ------------------------------------------------------------------------------------------------
# band pairs: partners a few fp32 ulps either side of eps
# ------------------------------------------------------------------------------------------------
BAND_STEPS = (-3, -2, -1, 0, 1, 2, 3)
BAND_SHAPE = (16, 96)


def _step(v, k):
    v = F32(v)
    for _ in range(abs(k)):
        v = np.nextafter(v, F32(np.inf if k > 0 else -np.inf))
    return v


def band_pairs(eps, min_points=4, seed=31):
    """One group per stepped axis (x, y) and step: min_points - 1 copies of a point p and one partner p + eps * e_k whose
    stepped coordinate is moved by -3 ... +3 fp32 ulps, so the partner decides whether the group is core (a cluster) or all of
    it noise.  p[k] = float32(0.25 * eps), which makes one ulp of the partner's coordinate about 3 * 2^-24 of eps; the other
    coordinates of p and its partner are equal.  Groups are 4 eps apart along the other axis.  Where float32(eps) == eps
    (1.5, 6, 40) the unmoved partner sits at d^2 == eps^2 exactly: that is the pair planted at equality (not a neighbour,
    the rule is strict); no other pair is.  Pixels are drawn at random over a 16 x 96 image, so a point and its partner
    usually sit in different tiles.
    -> (ri, tm, ground), facts: per group 'p', 'q', 'axis', 'step', the pixels of the group 'pix', 'd2f', 'in_band' (strictly
    between the screen's lo and hi), 'd2', 'neighbour' (the fp64 rule), 'fp32_neighbour' (d2f < float32(eps^2)), 'planted'
    (d2 == eps^2)."""
    H, W = BAND_SHAPE
    rng = np.random.default_rng(seed)
    eps = float(eps)
    e2 = eps * eps
    lo, hi = screen_bounds(eps)
    groups = []
    for g in range(2 * len(BAND_STEPS)):
        k, step = g // len(BAND_STEPS), BAND_STEPS[g % len(BAND_STEPS)]
        p = np.zeros(3, F32)
        p[1 - k] = F32(4.0 * eps * (g + 1))
        p[k] = F32(0.25 * eps)
        q = p.copy()
        q[k] = _step(F32(float(p[k]) + eps), step)
        groups.append(dict(p=p, q=q, axis=k, step=step))
    ri, tm = ground_frame(H, W)
    pix = rng.choice(H * W, len(groups) * min_points, replace=False).reshape(len(groups), min_points)
    for g, px in zip(groups, pix):
        put_points(ri, tm, px[:-1], np.tile(g["p"], (min_points - 1, 1)))
        put_points(ri, tm, px[-1:], g["q"][None])
        g["pix"] = px
        g["d2f"] = d2f(g["p"], g["q"])
        g["in_band"] = bool(lo < g["d2f"] < hi)
        g["d2"] = float(d2_exact(g["p"], g["q"]))
        g["neighbour"] = bool(g["d2"] < e2)
        g["fp32_neighbour"] = bool(g["d2f"] < F32(e2))
        g["planted"] = bool(g["d2"] == e2)
    check_frame(ri, tm)
    return (ri, tm, GROUND.copy()), dict(eps=eps, min_points=min_points, lo=lo, hi=hi, groups=groups,
                                         exact_planted=float(F32(eps)) == eps)


def band_expected(facts):
    """Labels the specification gives the frame of band_pairs: groups whose partner is a neighbour are clusters, numbered by the
    lowest pixel (= rank) among them; every other real point is noise.  (With min_points == 1 every point is core by itself;
    the generator is not meant for it.)"""
    assert facts["min_points"] >= 2
    H, W = BAND_SHAPE
    seg = np.zeros(H * W, np.int64)
    core = [g for g in facts["groups"] if g["neighbour"]]
    for g in facts["groups"]:
        seg[g["pix"]] = 2
    for n, g in enumerate(sorted(core, key=lambda g: int(g["pix"].min()))):
        seg[g["pix"]] = n + 3
    return seg.reshape(H, W)


# ------------------------------------------------------------------------------------------------
# hand frames with more than TILE_LIST tiles
# ------------------------------------------------------------------------------------------------
WIDE_H, WIDE_W = 8, 32 * 1030   # T = 1030: tile t holds the columns 32 t ... 32 t + 31


def _wide_pix(row, tile, k=0):
    return row * WIDE_W + tile * TILE_C + k


def far_border(eps=1.5, min_points=4):
    """border_lowest across the tile list.  Chain A (five points 0.5 m apart, row 0) holds the lowest core ranks: cluster 0.  Its
    end point, the only core point of A within eps of the border point, sits in tile 1025; the rest of A in tile 1027.  Chain B
    (cluster 1, row 1) and the border point (row 2) share tile 0.  The border point has three neighbours counting itself and
    takes the lowest number among its core neighbours: cluster 0's.  -> (ri, tm, ground), facts."""
    ri, tm = ground_frame(WIDE_H, WIDE_W)
    A = [(10.0 - 0.5 * k, 0.0, 0.0) for k in range(5)]
    B = [(12.8 + 0.5 * k, 0.0, 0.0) for k in range(5)]
    pa = [_wide_pix(0, 1025, 3)] + [_wide_pix(0, 1027, k) for k in range(4)]
    pb = [_wide_pix(1, 0, k) for k in range(5)]
    border = _wide_pix(2, 0, 7)
    put_points(ri, tm, pa, A)
    put_points(ri, tm, pb, B)
    put_points(ri, tm, [border], [(11.4, 0.0, 0.0)])
    check_frame(ri, tm)
    want = np.zeros(WIDE_H * WIDE_W, np.int64)
    want[pa], want[pb], want[border] = 3, 4, 3
    tile = tile_index(WIDE_H, WIDE_W).reshape(-1)
    facts = dict(T=tile_count(WIDE_H, WIDE_W), eps=eps, min_points=min_points, border=border, border_tile=int(tile[border]),
                 a_end=pa[0], a_end_tile=int(tile[pa[0]]), b_tile=int(tile[pb[0]]), want=want.reshape(WIDE_H, WIDE_W))
    return (ri, tm, GROUND.copy()), facts


ORIGIN_DIRS = ((1.4, 0.0, 0.0), (-1.4, 0.0, 0.0), (0.0, 1.4, 0.0), (0.0, -1.4, 0.0), (0.0, 0.0, 1.4))


def origin_company(Z, near, min_points, eps=1.5):
    """Z zero-range pixels spread over both halves of the tile range, `near` (<= 5) real points within eps of the origin but not
    of one another in tiles >= TILE_LIST, and a cluster of min_points copies of a far point in tile 0 (lower ranks than the
    origin's: cluster 0).  The origin point has Z + near neighbours; a near point has 1 + Z.  With Z + near >= min_points the
    origin is core (cluster 1) and the near points belong to it (as border points when 1 + Z < min_points); otherwise they
    are noise.  -> (ri, tm, ground), facts."""
    assert 1 <= Z and 0 <= near <= len(ORIGIN_DIRS)
    ri, tm = ground_frame(WIDE_H, WIDE_W)
    far = [_wide_pix(0, 0, k) for k in range(min_points)]
    put_points(ri, tm, far, np.tile([30.0, 0.0, 0.0], (min_points, 1)))
    T = tile_count(WIDE_H, WIDE_W)
    ztiles = np.linspace(1, T - 1, Z).astype(int)          # both halves of the tile range, the first after the far cluster
    zpix = [_wide_pix(1 + i % 7, int(t), 5) for i, t in enumerate(ztiles)]
    put_zero_range(ri, tm, zpix)
    npix = [_wide_pix(3, TILE_LIST + 1 + i, 2 + i) for i in range(near)]
    put_points(ri, tm, npix, np.array(ORIGIN_DIRS[:near], F32).reshape(-1, 3))
    check_frame(ri, tm)
    core = Z + near >= min_points
    want = np.zeros(WIDE_H * WIDE_W, np.int64)
    want[far] = 3
    want[npix] = 4 if core else 2
    want[zpix] = 1
    tile = tile_index(WIDE_H, WIDE_W).reshape(-1)
    facts = dict(T=T, eps=eps, min_points=min_points, Z=Z, near=near, origin_core=core, zero_tiles=tile[zpix], near_tiles=tile[npix],
                 want=want.reshape(WIDE_H, WIDE_W))
    return (ri, tm, GROUND.copy()), facts


ORIGIN_CASES = ((6, 3, 10), (7, 3, 10), (3, 5, 8), (12, 2, 10))   # (Z, near, min_points): one below the flip, the others at or past it


# ------------------------------------------------------------------------------------------------
# kNN ties: the integer grid
# ------------------------------------------------------------------------------------------------
KNN_SHAPES = ((16, 96), (300, 64))
KNN_RADII = (1.0, 2.0, 3.0, 2.0 ** 0.5, 5.0 ** 0.5)   # float32(r*r) of the last two is exactly 2 and exactly 5
KNN_K = 12


def knn_ties(H, W):
    """The integer grid of test_nn_adversarial_clouds: pixel (h, w) holds (w + 1, h + 1, 2), so every squared distance is a small
    integer, exact in fp32.  -> p f32 [H,W,3], facts."""
    assert float(F32(KNN_RADII[3] * KNN_RADII[3])) == 2.0 and float(F32(KNN_RADII[4] * KNN_RADII[4])) == 5.0
    g = np.stack(np.meshgrid(np.arange(W, dtype=F32), np.arange(H, dtype=F32)), -1)
    p = np.concatenate([g + 1, np.full((H, W, 1), 2.0, F32)], -1)
    check_eval_cloud(p, np.ones((H, W), bool))
    return p, dict(T=tile_count(H, W), radii=KNN_RADII)


def knn_tie_facts(p, r, k=KNN_K):
    """(queries with more than k points within r and a tie for the k-th place, queries with a candidate at d == float32(r*r)),
    by brute force over the integer grid (distances depend on the pixel offsets only)."""
    H, W = p.shape[:2]
    r2 = F32(r * r)
    R = int(np.floor(np.sqrt(float(r2)))) + 1
    cnt_tie, cnt_edge = 0, 0
    offs = [(dy, dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1)]
    d = np.array([F32(dy * dy + dx * dx) for dy, dx in offs])
    for h in range(H):
        for w in (0, 1, 2, W // 2, W - 1):          # the columns away from the edges are all alike
            ok = np.array([0 <= h + dy < H and 0 <= w + dx < W for dy, dx in offs])
            dd = np.sort(d[ok & (d <= r2)])
            cnt_tie += int(dd.size > k and dd[k - 1] == dd[k])
            cnt_edge += int(np.any(dd == r2))
    return cnt_tie, cnt_edge


# ------------------------------------------------------------------------------------------------
# flat lists for calc_chamfer_distance
# ------------------------------------------------------------------------------------------------
FLAT_N = (300000, 280000)


def flat_lists(seed=41):
    """Two shuffled [N,3] lists of 300 000 and 280 000 points, the second a 0.02 m jittered copy of part of the first: through
    evaluate_metrics' folding to rows of 2048 points they have H = 147 and T = 19 * 64 = 1216 tiles."""
    rng = np.random.default_rng(seed)
    n1, n2 = FLAT_N
    a = _blob_cloud(rng, n1, blobs=200)
    b = (a[rng.permutation(n1)[:n2]] + rng.normal(0, 0.02, (n2, 3))).astype(F32)
    assert eval_valid(a).all() and eval_valid(b).all()
    H = -(-n1 // 2048)
    return (a, b), dict(H=H, W=2048, T=tile_count(H, 2048))
