"""The scenes of tests/assign_sums_cases.py hold what their cases are there for (CPU: numpy and the oracle)."""
import numpy as np

import assign_sums_cases as ac


def _frames(name):
    return list(zip(ac.CASES[name][3], ac.case_expected(name)))


def test_every_frame_has_cluster_pixels_and_the_frames_of_a_call_differ():
    """A sum that lands in another frame's row shows only if the frames' rows differ."""
    for name, (H, W, M, frames) in ac.CASES.items():
        es = ac.case_expected(name)
        for e in es:
            assert e["model"].shape[0] <= M + 2 and e["counts"][2:].sum() > 0, name
        for i in range(len(es)):
            for j in range(i + 1, len(es)):
                assert not np.array_equal(es[i]["model"][2:, 3].view(np.uint32)[:4], es[j]["model"][2:, 3].view(np.uint32)[:4]), (name, i, j)


def test_shapes_reach_the_partial_tiles_and_both_histogram_forms():
    H, W = ac.CASES["ragged"][:2]
    tiles = -(-H // ac.TILE_ROWS) * -(-W // ac.TILE_COLS)
    assert H % ac.TILE_ROWS and W % ac.TILE_COLS and tiles % 4 and H * W < 1024       # partial tiles, a padding wavefront, one ragged scatter tile
    H, W = ac.CASES["vector"][:2]
    assert H % ac.TILE_ROWS == 0 and W % ac.TILE_COLS == 0 and (H * W) % 4 == 0 and H * W > 4 * 1024
    H, W = ac.CASES["w2250"][:2]
    assert (H, W) == (8, 2250) and W % ac.TILE_COLS
    for name in ("scalar", "mixed-scalar"):
        H, W = ac.CASES[name][:2]
        assert (H * W) % 4 != 0, name                                                 # hist_vec: the element-wise form
    assert ac.CASES["uint16"][2] > 254 and ac.CASES["uint16"][2] <= 510               # uint16 labels, eight screening rounds
    assert len({ac.CASES[n][2] for n, _, _ in ac.MIXED}) == 1                          # one cluster count per mixed call


def test_window_frame_leaves_the_window_on_both_sides_and_only_it_does():
    for name in ac.CASES:
        for (kind, k), e in _frames(name):
            below, above = ac.outside_window(e)
            if kind == "window":
                assert below > 0 and above > 0, (name, k)
                # the oracle's rows of the labels concerned are the reference's sequential float64 sums
                r, s = e["ri"].reshape(-1), e["seg"].reshape(-1)
                for lab in sorted(set(s[(s >= 2) & ((r < ac.WINDOW_LO) | (r >= ac.WINDOW_HI))].tolist())):
                    assert e["model"][lab, 3].view(np.uint32) == ac.sequential_mean(e, lab).view(np.uint32), (name, lab)
            else:
                assert below == 0 and above == 0, (name, kind, k)


def test_packed_tile_holds_more_than_three_cluster_labels():
    H, W, M, frames = ac.CASES["packed"]
    for (kind, k), e in _frames("packed"):
        if kind in ("packed", "hollow"):
            assert len(ac.tile_cluster_labels(e, *ac.PACKED_TILE)) > 3, kind
            out = e["seg"].copy()
            out[ac.PACKED_TILE] = 0
            assert not (out >= 2).any(), kind                                          # every cluster pixel lies in that tile


def test_empty_labels_on_both_label_types():
    for name, kind in (("packed", "hollow"), ("uint16", "synth")):
        hit = [e for (kd, k), e in _frames(name) if kd == kind and ac.empty_labels(e)]
        assert hit, name
        e = hit[0]
        lab = ac.empty_labels(e)[0]
        assert lab < e["model"].shape[0] and e["model"][lab, 3].view(np.uint32) == ac.NAN_ROW, name
