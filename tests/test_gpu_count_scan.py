"""-m gpu: the label counts of the ordered scatter, whichever launch makes them -- count_scan_kernel (the frame's one workgroup counts its
tiles into LDS and scans them there) or the histogram + scan pair that larger tables keep (launch_point_model, r-pcc_amd/csrc/rpcc_hip.hip).

Seen through the public entries on byte labels: ops.predict_quantize on a caller's integer residual with a step of 1 must leave the residual
stable-sorted by label without label 1, and nnz = P - (pixels of label 1); ops.decode of that list must put every value back on its pixel.
The reference is this file's own: per-tile bincounts, the labels' bases, the tiles' offsets -- the three things the kernel computes."""
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TILE = 1024
HIP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "r-pcc_amd", "csrc", "rpcc_hip.hip")


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    import rpcc_amd  # noqa: F401
    from rpcc_amd import ops
    return dict(torch=torch, ops=ops, dev=torch.device("cuda:0"))


# ------------------------------------------------------------------------------------------------
# the launch rule, restated from the source's one statement of it
# ------------------------------------------------------------------------------------------------
def lds_budget():
    m = re.search(r"size_t count_scan_lds_budget\(\) \{ return \(size_t\)(\d+) \* 1024; \}", open(HIP).read())
    assert m, "count_scan_lds_budget() not found in rpcc_hip.hip"
    return int(m.group(1)) * 1024


def lds_bytes(P, M):
    """count_scan_lds_bytes: a row of K 16-bit counts per tile, two to a word, the whole rounded up to 16 bytes."""
    return -(-(-(-P // TILE) * ((M + 3) // 2) * 4) // 16) * 16


def fused(P, M):
    return lds_bytes(P, M) <= lds_budget()


# ------------------------------------------------------------------------------------------------
# reference
# ------------------------------------------------------------------------------------------------
def reference(seg, K):
    """seg u8 [P] -> (offset [T, K], nnz, pos [P]): per-tile bincount; base = exclusive cumulative sum of the label totals with label 1
    zeroed; offset[t, k] = base[k] + pixels of label k in the tiles before t; nnz = P - pixels of label 1; pos[p] = the place of pixel p
    in the label-ordered list (offset of its tile and label + the pixels of that label before it in the tile), -1 for label 1."""
    P = seg.size
    T = -(-P // TILE)
    cnt = np.stack([np.bincount(seg[t * TILE:(t + 1) * TILE], minlength=K)[:K] for t in range(T)]).astype(np.int64)
    tot = cnt.sum(axis=0)
    live = tot.copy()
    live[1] = 0
    base = np.cumsum(live) - live
    offset = base[None, :] + np.cumsum(cnt, axis=0) - cnt
    pos = np.full(P, -1, np.int64)
    for t in range(T):
        lt = seg[t * TILE:(t + 1) * TILE].astype(np.int64)
        order = np.argsort(lt, kind="stable")
        first = np.cumsum(cnt[t]) - cnt[t]                     # start of each label inside the tile's sorted pixels
        rank = np.empty(lt.size, np.int64)
        rank[order] = np.arange(lt.size) - first[lt[order]]
        pos[t * TILE:t * TILE + lt.size] = offset[t, lt] + rank
    pos[seg == 1] = -1
    return offset, int(P - tot[1]), pos


def residual_of(B, P):
    """Integer-valued, inside int16, and telling neighbouring pixels and frames apart."""
    p = np.arange(P, dtype=np.int64)
    return np.stack([((p * 7 + b * 4099) % 40009 - 20004) for b in range(B)]).astype(np.float32)


def expected(seg, R, K):
    """-> (q [B, P] with zeros behind nnz, nnz [B], rec [B, P])."""
    B, P = seg.shape
    q, nnz, rec = np.zeros((B, P), np.int16), np.zeros(B, np.int32), np.zeros((B, P), np.float32)
    for b in range(B):
        _, n, pos = reference(seg[b], K)
        keep = pos >= 0
        assert n == int(keep.sum()) and np.array_equal(np.sort(pos[keep]), np.arange(n))
        q[b, pos[keep]] = R[b, keep].astype(np.int16)
        # the same list, said the other way: a stable sort by label, label 1 left out
        order = np.argsort(seg[b], kind="stable")
        order = order[seg[b, order] != 1]
        assert np.array_equal(q[b, :n], R[b, order].astype(np.int16))
        nnz[b] = n
        rec[b, keep] = R[b, keep]
    return q, nnz, rec


def device_labels(env, seg, shift=0):
    """seg [B, P] on the device; shift: bytes by which its first label is off a 16-byte boundary."""
    torch = env["torch"]
    B, P = seg.shape
    raw = torch.zeros(B * P + 16, dtype=torch.uint8, device=env["dev"])
    assert raw.data_ptr() % 16 == 0
    d = raw[shift:shift + B * P].view(B, P)
    d.copy_(torch.from_numpy(np.ascontiguousarray(seg)))
    assert d.data_ptr() % 16 == shift % 16
    return d


def run(env, seg, M, shift=0, ws=None, cws=None):
    """predict_quantize on the residual, then decode of its list: both against the reference."""
    torch, ops, dev = env["torch"], env["ops"], env["dev"]
    B, P = seg.shape
    K = M + 2
    assert seg.dtype == np.uint8 and int(seg.max()) < K
    R = residual_of(B, P)
    want_q, want_nnz, want_rec = expected(seg, R, K)
    d_seg = device_labels(env, seg, shift)
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
    d_tm, d_model = z(P, 3), z(B, K, 4)
    q, nnz, _ = ops.predict_quantize(z(B, P), d_tm, d_seg, d_model, 1.0, M, int16=True, residual=torch.from_numpy(R).to(dev), ws=ws)
    rec, _ = ops.decode(d_seg.view(B, 1, P), q, d_model, d_tm, 1.0, ws=cws)
    torch.cuda.synchronize()
    tag = (B, P, M, shift, fused(P, M))
    assert np.array_equal(nnz.cpu().numpy(), want_nnz), (tag, nnz.cpu().numpy(), want_nnz)
    got = q.cpu().numpy()
    bad = np.flatnonzero(got != want_q)
    assert bad.size == 0, (tag, bad.size, bad[:8], got.reshape(-1)[bad[:8]], want_q.reshape(-1)[bad[:8]])
    got = rec.cpu().numpy().reshape(B, P)
    bad = np.flatnonzero(got != want_rec)
    assert bad.size == 0, (tag, "decode", bad.size, bad[:8], got.reshape(-1)[bad[:8]], want_rec.reshape(-1)[bad[:8]])
    return q


def runs_of_labels(rng, B, P, K, mean_run=40):
    """Random labels in spatial runs (a lidar row's look): run lengths geometric around mean_run, about one run in eight empty (label 1)."""
    out = np.empty((B, P), np.uint8)
    for b in range(B):
        n = P // 4 + 8
        lens = rng.geometric(1.0 / mean_run, size=n)
        labs = rng.integers(0, K, size=n)
        labs[rng.random(n) < 0.125] = 1
        out[b] = np.repeat(labs, lens)[:P]
    return out


# ------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "off-by-one-byte"])
@pytest.mark.parametrize("P", [1000, 1024, 1025, 1028, 4 * 1024 + 4])
def test_tile_shapes(env, P, shift):
    """One partial tile, one whole tile, whole tiles and a short tail, P % 4 != 0 (the frames after the first start off every boundary), and
    a label map whose first byte is off the 16-byte boundary: the 16-byte loads, the byte loads and the switch between them inside a frame."""
    rng = np.random.default_rng(100 + P)
    run(env, runs_of_labels(rng, 2, P, 22, mean_run=9), 20, shift=shift)


@pytest.mark.parametrize("T", [5, 33, 65, 129])
def test_trip_counts(env, T):
    """Fewer tiles than wavefronts, one more than a whole round of wavefronts x loads in flight (32 tiles with four wavefronts, 64 with the
    eight the kernel has), and an odd tail behind whole rounds -- three different frames, the last tile partial."""
    rng = np.random.default_rng(200 + T)
    run(env, runs_of_labels(rng, 3, T * TILE - 24, 102), 100)


def test_one_label_fills_every_tile(env):
    """1024 pixels of one cluster label in every tile: the largest value of a 16-bit table entry, in an odd and in an even label (the two
    halves of a word)."""
    for lab in (5, 6):
        run(env, np.full((1, 3 * TILE), lab, np.uint8), 100)


def test_every_pixel_empty(env):
    """Label 1 alone: nnz = 0 and nothing in the list."""
    q = run(env, np.ones((2, 2 * TILE + 100), np.uint8), 100)
    assert not q.cpu().numpy().any()


def test_256_labels_in_a_tile(env):
    """Labels cycling 0 .. 255 pixel by pixel at 254 clusters: every tile (and every lane's 16 pixels) holds many labels, none may be left
    to a capped round."""
    P = 4 * TILE + 100
    run(env, (np.arange(2 * P) % 256).astype(np.uint8).reshape(2, P), 254)


def test_one_cluster(env):
    rng = np.random.default_rng(3)
    run(env, rng.integers(0, 3, size=(2, 2 * TILE + 7)).astype(np.uint8), 1)


def test_labels_in_the_last_tile_only(env):
    seg = np.zeros((2, 6 * TILE + 300), np.uint8)
    seg[0, 6 * TILE:] = (np.arange(300) % 99) + 2
    seg[1, 6 * TILE + 150:] = 101
    run(env, seg, 100)


def test_random_runs_full_width(env):
    """Spatial runs over all 102 labels, two frames of 40 tiles."""
    rng = np.random.default_rng(4)
    run(env, runs_of_labels(rng, 2, 40 * TILE, 102), 100)


def test_workspace_contents_do_not_matter(env):
    """The workspaces filled with 0xFF, and holding what a call at another (P, M) left: the same results (run() checks each call)."""
    torch, ops, dev = env["torch"], env["ops"], env["dev"]
    rng = np.random.default_rng(5)
    big, small = (2, 9 * TILE + 40, 254), (2, 5 * TILE + 12, 37)
    ws, cws = ops.workspace(big[0], big[1], big[2], dev), ops.codec_workspace(big[0], big[1], big[2], dev)
    assert ws.numel() >= ops.workspace(*small, dev).numel() and cws.numel() >= ops.codec_workspace(*small, dev).numel()
    seg_big, seg_small = runs_of_labels(rng, big[0], big[1], big[2] + 2), runs_of_labels(rng, small[0], small[1], small[2] + 2)
    ws.fill_(0xFF)
    cws.fill_(0xFF)
    run(env, seg_small, small[2], ws=ws, cws=cws)
    run(env, seg_big, big[2], ws=ws, cws=cws)     # over the small call's leftovers
    run(env, seg_small, small[2], ws=ws, cws=cws)  # and the other way round


def test_launch_rule(env):
    """The largest image whose table fits the LDS budget at 254 clusters, one tile more (the two-launch path), and one 128 x 4096 frame at
    100 clusters (the two-launch path at the headline's cluster count): each equals the reference."""
    rng = np.random.default_rng(6)
    M = 254
    T = lds_budget() // (((M + 3) // 2) * 4)
    assert fused(T * TILE, M) and not fused(T * TILE + 1, M)
    assert fused(64 * 2048, 100) and fused(64 * 2048, 254) and fused(80 * 2000, 254) and not fused(128 * 4096, 100)
    run(env, runs_of_labels(rng, 1, T * TILE, M + 2), M)
    run(env, runs_of_labels(rng, 1, T * TILE + 4, M + 2), M)
    run(env, runs_of_labels(rng, 1, 128 * 4096, 102), 100)
