"""Hand-made inputs of rpcc_compress_batch_labels (include/rpcc_hip.h): int32 label maps in rpcc_seg_dbscan's convention -- ground 0,
ri == 0 pixels 1, noise 2, clusters from 3 -- as column stripes, built for what the label intake and the kernels behind it can get wrong:
a frame that reaches the cap's last label, labels above 255, runs of unused labels, frames without clusters, a top label without pixels,
ranges outside the point model's fixed-point window.  Every builder returns its claims (`facts`), and check_frame() holds them on the CPU
(tests/test_labels_abi.py), so a GPU comparison that passes has run the cases it names."""
import numpy as np

F32 = np.float32
SHAPES = ((16, 128), (10, 70), (9, 35), (64, 512))   # 10 x 70: H % 8, W % 32 != 0; 9 x 35: P % 4 != 0 (the non-vector intake); 64 x 512: 32 tiles
CAPS = (254, 1022)                                    # M: byte labels up to 255, uint16 labels up to 1023

# per cap, the three frames of a batch: (labels in use besides 1, max_label).  `use` cycles over the columns.
FRAMES = {
    254: (((0, 2, 3, 7, 40, 41, 200, 255), 255),       # reaches M + 1 exactly; runs of unused labels below the maximum
          ((0, 2), 2),                                  # ground, empty and noise only
          ((0, 3, 5, 17), 30)),                         # the top label has no pixel: max_label above the largest label present
    1022: (((0, 2, 3, 256, 300, 511, 512, 1000, 1023), 1023),   # reaches M + 1 exactly; labels >= 256
           ((0,), 0),                                   # max_label = 0: ground only, no empty pixel
           ((0, 2, 260, 700), 800)),                    # labels >= 256 with an unused top label
}


def rays(H, W):
    """A ray table f32 [H,W,3] of unit vectors (a 360 degree sweep, 2 .. -24.9 degrees: the formula of dataset/transformer.py:41-54)."""
    alt = np.deg2rad(-24.9 + 26.9 * np.arange(H) / max(H - 1, 1))
    azi = 2 * np.pi * np.arange(W) / W
    tm = np.zeros((H, W, 3))
    tm[..., 0] = np.cos(alt)[:, None] * np.cos(azi)[None, :]
    tm[..., 1] = np.cos(alt)[:, None] * np.sin(azi)[None, :]
    tm[..., 2] = np.sin(alt)[:, None]
    return tm.astype(F32)


def stripe_frame(H, W, use, max_label, seed, nonfinite=False):
    """-> (ri f32 [H,W], labels i32 [H,W], facts).  Column c carries use[c % len(use)], two columns wide; ranges 2 .. 60 m with a gentle
    trend per label (so that models and residuals are not trivial); where max_label >= 1, about one pixel in nine is empty (ri == 0,
    label 1).  nonfinite: one cluster pixel gets an infinite range and one NaN (the point model's sequential fallback)."""
    rng = np.random.default_rng(seed)
    lab = np.empty((H, W), np.int32)
    for c in range(W):
        lab[:, c] = use[(c // 2) % len(use)]
    ri = (2.0 + 55.0 * rng.random((H, W)) * 0.1 + (lab % 13) * 4.0).astype(F32)
    if max_label >= 1:
        empty = rng.random((H, W)) < 0.11
        empty[0, 0] = True
        ri[empty] = 0.0
        lab[empty] = 1
    facts = dict(max_label=int(max_label), used=sorted(set(int(v) for v in np.unique(lab))), nonfinite=[])
    if nonfinite:
        cl = np.argwhere(lab >= 3)
        assert cl.shape[0] >= 2, "no cluster pixel to make non-finite"
        (r0, c0), (r1, c1) = cl[len(cl) // 3], cl[2 * len(cl) // 3]
        ri[r0, c0], ri[r1, c1] = np.inf, np.nan
        facts["nonfinite"] = [(int(r0), int(c0)), (int(r1), int(c1))]
    facts["empty_labels"] = [k for k in range(max_label + 1) if k not in facts["used"]]
    return ri, lab, facts


def batch(H, W, cap, nonfinite=False, seed=0):
    """B = 3 frames with three different max_label under the label cap `cap` (M).
    -> dict(ri f32 [3,H,W], tm f32 [H,W,3], ground f64 [3,4], labels i32 [3,H,W], max_label i32 [3], frame_ids i64 [3], facts [3])."""
    ris, labs, facts = [], [], []
    for i, (use, mx) in enumerate(FRAMES[cap]):
        # (the non-finite ranges go to the last frame, whose clusters are labels 3 .. / 260 ..)
        ri, lab, f = stripe_frame(H, W, use, mx, seed=1000 * cap + 10 * seed + i, nonfinite=nonfinite and i == 2)
        ris.append(ri); labs.append(lab); facts.append(f)
    ground = np.array([[0.01, -0.02, -0.9997, -1.72], [-0.01, 0.005, -0.9999, -1.75], [0.0, 0.0, -1.0, -1.6]], np.float64)
    return dict(ri=np.stack(ris), tm=rays(H, W), ground=ground, labels=np.stack(labs), max_label=np.array([f["max_label"] for f in facts], np.int32),
                frame_ids=np.array([11, 5, 70007], np.int64), facts=facts, cap=cap)


def check_frame(ri, lab, facts, cap):
    """The claims of a frame, held on the CPU."""
    assert lab.dtype == np.int32 and ri.dtype == F32 and ri.shape == lab.shape
    assert np.array_equal(lab == 1, ri == 0), "label 1 exactly on ri == 0"
    mx = facts["max_label"]
    assert 0 <= lab.min() and lab.max() <= mx <= cap + 1
    for k in facts["empty_labels"]:
        assert not (lab == k).any(), k
    assert sorted(set(range(mx + 1)) - set(facts["empty_labels"])) == facts["used"]
    for (r, c) in facts["nonfinite"]:
        assert lab[r, c] >= 3 and not np.isfinite(ri[r, c])
    if facts["nonfinite"]:
        assert np.isinf(ri[facts["nonfinite"][0]]) and np.isnan(ri[facts["nonfinite"][1]])
    fin = np.isfinite(ri)
    assert (ri[fin] >= 0).all() and (ri[fin & (ri != 0)] >= 2.0).all() and (ri[fin] < 60.0).all()


def refusals(cap):
    """The middle frame of a 16 x 128 batch made unacceptable, in turn: (name, max_label of frame 1 or None to keep it, (pixel, label) to plant
    or None, expected status name).  Every planted label keeps max_label <= M + 1."""
    return (("max_label_above_cap", cap + 2, None, "LABELS_E_RANGE"),
            ("capped", -1, None, "LABELS_E_CAPPED"),
            ("negative_max_label", -5, None, "LABELS_E_RANGE"),
            ("label_above_cap", None, ((3, 77), cap + 2), "LABELS_E_RANGE"),
            ("negative_label", None, ((15, 127), -3), "LABELS_E_RANGE"))


MANY_GROUND = np.array([0.0, 0.0, -1.0, -1.7])   # the plane the frame below stands on (given to the compressor, not fitted)
MANY_MIN_LABEL = 60                                # its largest DBSCAN label is at least this (eps 1.5, min_points 10: test_labels_abi.py)


def vlp16_many_clusters(seed=3, spacing=3.0):
    """A sweep on which DBSCAN (eps 1.5, min_points 10) finds many clusters in the VLP-16 geometry (16 x 1800, +-15 degrees): posts
    0.4 m wide, `spacing` metres apart on rings of 8, 13 and 18 m around the sensor, from 1.2 m below the sensor's height up (no ground
    returns: the posts must not join through them).  -> xyz f32 [N,3]."""
    rng = np.random.default_rng(seed)
    pts = []
    for ring in (8.0, 13.0, 18.0):
        k = int(2 * np.pi * ring / spacing)
        for a in 2 * np.pi * (np.arange(k) + 0.37 * ring) / k:
            n = 400
            pts.append(np.stack([ring * np.cos(a) + rng.uniform(-0.2, 0.2, n), ring * np.sin(a) + rng.uniform(-0.2, 0.2, n),
                                 rng.uniform(-1.2, 1.5, n)], 1))
    return np.concatenate(pts).astype(F32)
