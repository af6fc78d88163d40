"""numpy reference of the DBSCAN segmentation.  No scipy or sklearn: the GPU machines may not have
them.  It follows the specification step by step, with a different search than the kernels:

* the non-ground mask in fp64, (a*A + b*B) + c*C as numpy sums the reference's plane products, a NaN residual is ground;
* points ri * tm in fp32, ranked row-major over the non-ground pixels;
* the zero-range non-ground pixels are one point at the origin with multiplicity Z (exact duplicates);
* neighbours from grid buckets of side eps, kept when ((dx*dx) + (dy*dy)) + (dz*dz) < eps*eps in fp64, the point itself
  counted;
* core points: at least min_points neighbours; clusters: components of core points, numbered by their lowest core rank;
* a border point takes the lowest cluster number among its core neighbours, otherwise it is noise;
* labels: ground 0, noise 2, cluster k -> k + 3, then every ri == 0 pixel 1."""
import numpy as np

CHUNK = 8192


def nonground(ri, tm, ground):
    """bool [H,W]: |double(ri) - r_plane| > 0.5, r_plane = -d / ((a*A + b*B) + c*C) in fp64 (NaN: ground)."""
    a, b, c, d = (float(v) for v in np.asarray(ground, np.float64))
    t = np.asarray(tm, np.float64)
    den = (a * t[..., 0] + b * t[..., 1]) + c * t[..., 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        res = np.asarray(ri, np.float32).astype(np.float64) - (-d / den)
        return np.abs(res) > 0.5


def points(ri, tm):
    return np.asarray(ri, np.float32)[..., None] * np.asarray(tm, np.float32)


def d2(p, q):
    """exact fp64 test quantity: dx = double(xp) - double(xq), ((dx*dx) + (dy*dy)) + dz*dz, un-fused."""
    dx = p[..., 0] - q[..., 0]
    dy = p[..., 1] - q[..., 1]
    dz = p[..., 2] - q[..., 2]
    return (dx * dx + dy * dy) + dz * dz


class _Grid:
    """Real points bucketed in cubes of side eps: every neighbour of a point lies in the 27 cubes around its own."""

    def __init__(self, pts, eps):
        self.p = pts
        with np.errstate(invalid="ignore", over="ignore"):
            cell = np.floor(pts / eps)
        cell = np.where(np.isfinite(cell), cell, 0).astype(np.int64)
        self.cell = cell
        lo = cell.min(0) - 1 if len(cell) else np.zeros(3, np.int64)
        self.lo, self.dim = lo, (cell.max(0) - lo + 2) if len(cell) else np.ones(3, np.int64)
        key = self._key(cell)
        self.order = np.argsort(key, kind="stable")
        self.skey = key[self.order]

    def _key(self, c):
        c = c - self.lo
        return (c[:, 0] * self.dim[1] + c[:, 1]) * self.dim[2] + c[:, 2]

    def pairs(self, qi):
        """(query index, candidate index) pairs of the query points qi over the 27 cubes; the exact test is left to the caller."""
        out_q, out_c = [], []
        for ox in (-1, 0, 1):
            for oy in (-1, 0, 1):
                for oz in (-1, 0, 1):
                    k = self._key(self.cell[qi] + np.array([ox, oy, oz]))
                    s = np.searchsorted(self.skey, k, "left")
                    e = np.searchsorted(self.skey, k, "right")
                    cnt = e - s
                    tot = int(cnt.sum())
                    if tot == 0:
                        continue
                    q = np.repeat(qi, cnt)
                    start = np.repeat(s - np.concatenate(([0], np.cumsum(cnt)[:-1])), cnt)
                    out_q.append(q)
                    out_c.append(self.order[start + np.arange(tot)])
        if not out_q:
            return np.zeros(0, np.int64), np.zeros(0, np.int64)
        return np.concatenate(out_q), np.concatenate(out_c)


def _find(parent, x):
    r = parent[x]
    while True:
        nr = parent[r]
        if np.array_equal(nr, r):
            return r
        r = nr


def _union(parent, u, v):
    """Hook the larger root onto the smaller until every edge (u, v) joins one tree (vectorised, order-free); parent is
    updated in place and left fully compressed."""
    while len(u):
        ru, rv = _find(parent, u), _find(parent, v)
        m = ru != rv
        if not m.any():
            return
        u, v, ru, rv = u[m], v[m], ru[m], rv[m]
        np.minimum.at(parent, np.maximum(ru, rv), np.minimum(ru, rv))
        while True:   # every node points at its root
            nxt = parent[parent]
            if np.array_equal(nxt, parent):
                break
            parent[:] = nxt


def dbscan_frame(ri, tm, ground, eps, min_points=10, with_clusters=False):
    """Final labels int64 [H,W] of one frame (optionally also the per-rank cluster numbers, -1 = noise, and the core flags)."""
    ri = np.asarray(ri, np.float32)
    H, W = ri.shape
    ng = nonground(ri, tm, ground).reshape(-1)
    pix = np.nonzero(ng)[0]                       # rank -> pixel
    n = pix.size
    r_flat = ri.reshape(-1)[pix]
    origin = r_flat == 0
    Z = int(origin.sum())
    o0 = int(np.argmax(origin)) if Z else -1      # lowest origin rank
    real = np.nonzero(~origin)[0]                 # ranks of the real points
    P = points(ri, tm).reshape(-1, 3)[pix[real]].astype(np.float64)
    e2 = float(eps) * float(eps)
    g = _Grid(P, float(eps))
    near_o = d2(P, np.zeros(3)) < e2
    m = len(real)

    # core flags
    cnt = np.zeros(m, np.int64)
    for c0 in range(0, m, CHUNK):
        q, c = g.pairs(np.arange(c0, min(m, c0 + CHUNK)))
        hit = d2(P[q], P[c]) < e2
        cnt += np.bincount(q[hit], minlength=m)[:m] if len(q) else 0
    cnt += Z * near_o
    core_r = cnt >= min_points
    core_o = Z > 0 and Z + int(near_o.sum()) >= min_points

    # components over core-core edges, on ranks
    parent = np.arange(n, dtype=np.int64)
    core = np.zeros(n, bool)
    core[real[core_r]] = True
    if core_o:
        core[o0] = True
    cidx = np.nonzero(core_r)[0]
    for c0 in range(0, len(cidx), CHUNK):
        q, c = g.pairs(cidx[c0:c0 + CHUNK])
        keep = core_r[c] & (c < q)
        q, c = q[keep], c[keep]
        hit = d2(P[q], P[c]) < e2
        _union(parent, real[q[hit]], real[c[hit]])
    if core_o:
        s = real[core_r & near_o]
        _union(parent, s, np.full(s.size, o0, np.int64))
    root = _find(parent, np.arange(n))
    is_root = core & (root == np.arange(n))
    num = np.cumsum(is_root) - 1
    cl = np.where(core, num[root], -1)

    # border points: the lowest cluster number among core neighbours
    bidx = np.nonzero(~core_r)[0]
    best = np.full(m, np.iinfo(np.int64).max)
    if core_o:
        best[near_o] = cl[o0]
    for c0 in range(0, len(bidx), CHUNK):
        q, c = g.pairs(bidx[c0:c0 + CHUNK])
        keep = core_r[c]
        q, c = q[keep], c[keep]
        hit = d2(P[q], P[c]) < e2
        np.minimum.at(best, q[hit], cl[real[c[hit]]])
    bsel = real[bidx]
    cl[bsel] = np.where(best[bidx] == np.iinfo(np.int64).max, -1, best[bidx])

    seg = np.zeros(H * W, np.int64)
    seg[pix] = np.where(cl < 0, 2, cl + 3)
    seg[ri.reshape(-1) == 0] = 1
    seg = seg.reshape(H, W)
    if with_clusters:
        return seg, cl, core
    return seg


def sklearn_labels(ri, tm, ground, eps, min_points=10):
    """The reference's path (segment_utils.py:149-169) with sklearn's DBSCAN in place of Open3D's: an independent
    implementation (sklearn counts d <= eps; callers make sure no pair sits at d == eps)."""
    from sklearn.cluster import DBSCAN
    ri = np.asarray(ri, np.float32)
    ng = nonground(ri, tm, ground)
    pc = points(ri, tm)[ng]
    labels = DBSCAN(eps=eps, min_samples=min_points).fit(pc.astype(np.float64)).labels_ if len(pc) else np.zeros(0, np.int64)
    # sklearn numbers clusters by the expansion order from the lowest-index unvisited core point, which is the lowest core rank
    seg = np.zeros(ri.shape, np.int64)
    seg[ng] = labels + 2
    seg[seg > 0] += 1
    seg[ri == 0] = 1
    return seg


# ------------------------------------------------------------------------------------------------
# hand fixtures: frames built pixel by pixel.  With the ground plane GROUND = (0, 0, 1, 1), a pixel whose ray has z = 0 is
# non-ground whatever its range (r_plane = -1 / 0 = -inf), and a pixel with ray (0, 0, -1) and range 1 is ground
# (r_plane = 1).  A real point p is the pixel (ri = 1, tm = p); a zero-range point the pixel (ri = 0, tm = (1, 0, 0)).
# ------------------------------------------------------------------------------------------------
GROUND = np.array([0.0, 0.0, 1.0, 1.0])
FIX_H, FIX_W = 8, 64


def frame(entries, H=FIX_H, W=FIX_W):
    """entries: row-major pixels, each ('p', (x, y, z)) real point with z = 0, ('o',) zero-range non-ground, ('g',) ground,
    ('g0',) zero-range ground-ray pixel; every later pixel is ground.  -> (ri f32 [H,W], tm f32 [H,W,3])."""
    ri = np.ones(H * W, np.float32)
    tm = np.zeros((H * W, 3), np.float32)
    tm[:, 2] = -1.0
    assert len(entries) <= H * W
    for i, e in enumerate(entries):
        if e[0] == "p":
            assert e[1][2] == 0
            tm[i] = e[1]
        elif e[0] == "o":
            ri[i], tm[i] = 0.0, (1.0, 0.0, 0.0)
        elif e[0] == "g0":
            ri[i] = 0.0
    return ri.reshape(H, W), tm.reshape(H, W, 3)


def fixtures():
    """{name: (ri, tm, min_points, expected labels of the first len(entries) pixels)}: one rule each."""
    P = lambda x, y=0.0: ("p", (x, y, 0.0))   # noqa: E731
    out = {}
    # strict <: nine copies of a point and one at d^2 = 2.25 exactly are ten points but nobody has ten neighbours -> noise
    e = [P(10.0)] * 9 + [P(11.5)]
    out["boundary_strict"] = (*frame(e), 10, [2] * 10)
    e = [P(10.0)] * 9 + [P(11.4999)]
    out["boundary_inside"] = (*frame(e), 10, [3] * 10)
    # min_points counts the point itself: ten copies are core, nine are noise
    out["min_points_self"] = (*frame([P(5.0)] * 10 + [P(40.0)] * 9), 10, [3] * 10 + [2] * 9)
    # a border point between two clusters takes the lower number: B (ranks first) is cluster 0, A cluster 1
    B = [P(12.8 + 0.5 * k) for k in range(5)]
    A = [P(10.0 - 0.5 * k) for k in range(5)]
    out["border_lowest"] = (*frame(B + A + [P(11.4)]), 4, [3] * 4 + [3] + [4] * 4 + [4] + [3])
    # the origin cluster (twelve zero-range pixels, ranks first) is cluster 0: its pixels become 1 and label 3 stays empty
    out["origin_keeps_number"] = (*frame([("o",)] * 12 + [P(20.0)] * 10), 10, [1] * 12 + [4] * 10)
    # ground 0 (a zero-range ground-ray pixel 1), noise 2
    out["ground_noise"] = (*frame([("g",), ("g0",), P(30.0), ("g",)] + [P(50.0)] * 10), 10, [0, 1, 2, 0] + [3] * 10)
    return out
