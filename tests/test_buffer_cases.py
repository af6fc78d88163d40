"""The facts tests/buffer_cases.py claims about its batches, proved with the oracle alone (no GPU): a case cannot silently stop exercising
what it is for, and no frame lies where the reference leaves the result undefined -- so the device tests need not skip any."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import buffer_cases as C   # noqa: E402
from oracle import oracle as orc   # noqa: E402

SCENES = sorted(C.SEEDS)


def test_geometries_cross_the_seams():
    P = {n: h * w for n, (h, w, _, _) in C.GEOMETRIES.items()}
    assert 1024 < P["5x300"] <= 2048 and P["5x300"] % 64 != 0            # two scatter tiles, tile table unaligned
    assert 32768 < P["16x2101"] <= 65536 and P["16x2101"] % 64 != 0     # two projection bands
    assert P["16x1800"] == 28800 and P["16x1800"] % 64 == 0
    assert C.B == 6 and C.KINDS.count(C.ORDINARY) == 2 and C.KINDS.count(C.SALTED) == 2
    assert [b for b, k in enumerate(C.KINDS) if k == C.SALTED] == [1, 4]   # one odd, one even batch position
    for name, Ms in C.CLUSTERS.items():
        assert {7, 100, 254, 300} <= set(Ms) and ((C.RADIX_M in Ms) == (name == "5x300"))
    assert C.RADIX_M > 1022 and {C.scene_of(M) for M in (7, 100, 254, 300)} == {"default"}
    assert sorted({(n, C.scene_of(M)) for n, Ms in C.CLUSTERS.items() for M in Ms}) == SCENES


@pytest.mark.parametrize("name,scene", SCENES)
def test_frames_are_what_they_are_for(name, scene):
    g = C.geom_of(name)
    tm = orc.transform_map(g)
    fr = C.frames(name, scene)
    ris, gms = C.grounds(name, scene)
    assert len(fr) == C.B
    for b, kind in enumerate(C.KINDS):
        f = fr[b]
        if kind == C.EMPTY:
            assert f.shape == (0, 3) and not ris[b].any() and gms[b] is None
            continue
        assert np.isfinite(gms[b]).all()
        zero = ~f.any(1)
        if kind == C.SALTED:
            # the points at the origin really reset a pixel: without them the image differs, and only at pixels that lose their value or
            # fall back to a later, farther return
            assert int(zero.sum()) == 3 and zero[-1]
            plain = orc.project(f[~zero], g)
            d = np.flatnonzero(plain.reshape(-1) != ris[b].reshape(-1))
            assert d.size >= 1
            assert ((ris[b].reshape(-1)[d] == 0) | (ris[b].reshape(-1)[d] > plain.reshape(-1)[d])).all()
        else:
            assert not zero.any()
        cand = C.ground_candidates(ris[b], tm)
        if kind == C.GROUNDLESS:
            assert cand < 800, (name, scene, cand)          # the whole-cloud fit
        elif name != "5x300":
            assert cand >= 800, (name, scene, b, cand)      # (a 1500-pixel image never has 800 candidates: all its frames fit the whole cloud)
    assert any(C.ground_candidates(ris[b], tm) < 800 for b in range(C.B) if C.KINDS[b] != C.EMPTY)


@pytest.mark.parametrize("name,scene", SCENES)
def test_no_frame_outside_the_oracles_domain(name, scene):
    """Every non-empty frame has as many DISTINCT centre pixels as clusters, for every cluster count used with its geometry (otherwise the reference's
    centre list repeats and nothing downstream is defined)."""
    d, top = C.distinct_centres(name, scene)
    assert sorted(d) == [b for b in range(C.B) if C.KINDS[b] != C.EMPTY]
    assert top == max(M for M in C.CLUSTERS[name] if C.scene_of(M) == scene)
    assert all(n == top for n in d.values()), (name, scene, d)


@pytest.mark.parametrize("name,M,variant", [("5x300", 7, "uniform_point"), ("5x300", 300, "nonuniform_plane"), ("5x300", C.RADIX_M, "uniform_point")])
def test_expected_is_complete(name, M, variant):
    """The shared oracle results: one dict per non-empty frame, labels wide enough to need the label type the case is for."""
    exp = C.expected(name, M, variant)
    assert len(exp) == C.B and exp[2] is None and C.expected(name, M, variant) is exp
    for b, o in enumerate(exp):
        if o is None:
            continue
        assert len(set(o["fps_pix"].tolist())) == M
        assert o["q"].shape[0] == int((o["seg_idx"] != 1).sum())
        assert (o["salience"] is None) == (variant == "uniform_point")
        if M > 254:
            assert int(o["seg_idx"].max()) > 255
