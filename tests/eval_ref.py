"""numpy reference of the reconstruction metrics (DESIGN.md "Reconstruction metrics"): fp32 distances in the kernel's
operation order, lowest index among equal minima, fp64 sums.  No scipy: the GPU machines may not have it.

The searches are exact brute force over a candidate set.  A `hint` (e.g. the device's answer) only narrows that set: its
distance, recomputed here, bounds the true minimum from above, and every point within that bound survives the box filter
(fl(dx*dx) <= d, so |dx| <= sqrt(d) (1 + 2^-23)), so a wrong hint cannot make the reference agree with it."""
import numpy as np

F32 = np.float32


def compact(pts):
    """[..., 3] -> the valid points ((x + y) + z != 0 in fp32) in row-major order, f32 [N,3]."""
    p = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 3)
    return p[((p[:, 0] + p[:, 1]) + p[:, 2]) != 0]


def d2(q, s):
    """f32 [m,n]: ((dx*dx) + (dy*dy)) + (dz*dz), dx = q - s."""
    dx = q[:, None, 0] - s[None, :, 0]
    dy = q[:, None, 1] - s[None, :, 1]
    dz = q[:, None, 2] - s[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def d2_pairs(q, s):
    dx, dy, dz = q[:, 0] - s[:, 0], q[:, 1] - s[:, 1], q[:, 2] - s[:, 2]
    return (dx * dx + dy * dy) + dz * dz


def _candidates(qc, s64, bound):
    if not np.isfinite(bound):
        return np.arange(s64.shape[0])
    rad = np.sqrt(float(bound)) * (1 + 1e-6) + 1e-30
    q64 = qc.astype(np.float64)
    lo, hi = q64.min(0) - rad, q64.max(0) + rad
    return np.nonzero(np.all((s64 >= lo) & (s64 <= hi), axis=1))[0]


def nn(q, s, hint=None, chunk=256):
    """Nearest point of s for every point of q -> (dist f32 [m], idx int64 [m])."""
    m, n = q.shape[0], s.shape[0]
    dist, idx = np.empty(m, F32), np.empty(m, np.int64)
    s64 = s.astype(np.float64)
    for c0 in range(0, m, chunk):
        qc = q[c0:c0 + chunk]
        bound = np.inf
        if hint is not None:
            h = np.asarray(hint[c0:c0 + chunk], np.int64)
            if np.all((h >= 0) & (h < n)):
                bound = float(d2_pairs(qc, s[h]).max())
        sel = _candidates(qc, s64, bound)
        D = d2(qc, s[sel])
        a = np.argmin(D, axis=1)   # first minimum; sel is ascending -> lowest index
        dist[c0:c0 + chunk] = D[np.arange(len(qc)), a]
        idx[c0:c0 + chunk] = sel[a]
    return dist, idx


def knn(q, s, r, k=12, hint=None, chunk=128):
    """The <= k nearest points of s within d2 <= f32(r*r) (lowest index among ties) -> int64 [m,k], -1 padded."""
    r2 = F32(r * r)
    m, n = q.shape[0], s.shape[0]
    out = np.full((m, k), -1, np.int64)
    s64 = s.astype(np.float64)
    for c0 in range(0, m, chunk):
        qc = q[c0:c0 + chunk]
        bound = float(r2)
        if hint is not None:
            h = np.asarray(hint[c0:c0 + chunk], np.int64)
            if np.all((h >= 0) & (h < n)):   # k distinct points within the bound: the true k-th is no farther
                bound = min(bound, float(d2_pairs(np.repeat(qc, k, 0), s[h.reshape(-1)]).reshape(-1, k).max()))
        sel = _candidates(qc, s64, bound)
        D = d2(qc, s[sel])
        order = np.argsort(D, axis=1, kind="stable")[:, :k]
        Dk = np.take_along_axis(D, order, 1)
        res = np.where(Dk <= r2, sel[order], -1)
        out[c0:c0 + chunk, :res.shape[1]] = res
    return out


def normal_of(s, nbr_row):
    """(normal, eigenvalues, covariance) of the neighbour set by numpy.linalg.eigh (fp64); normal oriented n . p <= 0 by the caller."""
    pts = s[nbr_row[nbr_row >= 0]].astype(np.float64)
    c = pts - pts.mean(0)
    C = c.T @ c / pts.shape[0]
    w, v = np.linalg.eigh(C)
    return v[:, 0], w, C


def assign_attr(attr1, idx1, idx2):
    """utils/evaluate_metrics.py:101-117 restated: plain (un-renormalised) averages, sequential fp64 sums."""
    n2 = idx1.shape[0]
    counts = np.zeros(n2)
    sums = np.zeros((n2, attr1.shape[1]))
    np.add.at(counts, idx2, 1)
    np.add.at(sums, idx2, attr1)
    empty = counts == 0
    counts[empty] = 1
    sums[empty] = attr1[idx1[empty]]
    return sums / counts[:, None]


def d1_d2(pc1, pc2, nn12, nn21, n1):
    """(d1 mse_1, mse_2, d2 mse_1, mse_2) in fp64 from given indices (nn12: cloud-1 -> cloud-2) and cloud-1 normals."""
    n2 = assign_attr(n1, nn21, nn12)
    e1 = (pc1 - pc2[nn12])          # f32 differences, as numpy subtracts two float32 clouds
    e2 = (pc2 - pc1[nn21])
    d1 = (float(np.sum(d2_pairs(pc1, pc2[nn12]).astype(np.float64))) / pc1.shape[0],
          float(np.sum(d2_pairs(pc2, pc1[nn21]).astype(np.float64))) / pc2.shape[0])
    t1 = ((e1[:, 0] * n2[nn12, 0] + e1[:, 1] * n2[nn12, 1]) + e1[:, 2] * n2[nn12, 2]) ** 2
    t2 = ((e2[:, 0] * n1[nn21, 0] + e2[:, 1] * n1[nn21, 1]) + e2[:, 2] * n1[nn21, 2]) ** 2
    return d1[0], d1[1], float(t1.sum()) / pc1.shape[0], float(t2.sum()) / pc2.shape[0]
