#!/usr/bin/env python3
"""Fourth fixture: the reference's own C++ on the seeded inputs of tests/test_oracle_vs_ref.py -> tests/golden/ref_cpp_manifest.json.

Runs only in the build container (needs oracle/_ref, built by `make -C oracle ref` from the reference's sources).  The inputs come
from the test module's _*_inputs() helpers, so the test and this script cannot drift apart.  Every call of the reference runs in a
fresh process: it leaves the cells of feat / key_point_map it does not write uninitialised (cpp_modules.cpp:38-43), and outputs
of a fresh process are mmap'd zero pages.  Stored: SHA-256 digests of the reference's outputs (and of the inputs, as a guard),
in the dtypes the restatement returns; the test hashes the restatement's outputs the same way.  Nothing of the reference travels."""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REFDIR = os.path.join(ROOT, "oracle", "_ref")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402

from oracle import oracle as orc  # noqa: E402
import test_oracle_vs_ref as T  # noqa: E402

_CHILD = """
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
import dataset_utils_cpp as ds, segment_utils_cpp as sg, quantization_utils_cpp as q, feature_extractor_cpp as fe, contour_utils_cpp as ct
z = dict(np.load(sys.argv[2]))
g = z.get("geom")   # H, W, horizontal FOV, vertical max, vertical min
fn = {"project": lambda: [ds.point_cloud_to_range_image_even(z["xyz"], int(g[0]), int(g[1]), float(g[2]), float(g[3]), float(g[4]))],
      "point_modeling": lambda: [sg.point_modeling(z["ri"].reshape(z["ri"].shape + (1,)), z["seg"])],
      "intra_predict": lambda: [sg.intra_predict(z["seg"], z["mp"], z["tm"])],
      "uniform_quantize": lambda: [q.uniform_quantize(z["seg"], z["res"], float(z["acc"]) if "acc" in z else 0.04)],
      "nonuniform_quantize": lambda: list(q.nonuniform_quantize(z["seg"], z["res"], z["kp"], z["lk"], z["la"], int(z["gl"]) if "gl" in z else 2)),
      "features": lambda: list(fe.extract_features_with_segment(z["ri"], z["seg"], *[int(v) for v in z["params"]])),
      "contour": lambda: list(ct.extract_contour(z["seg"])),
      "recover_map": lambda: [ct.recover_map(z["cm"], z["sq"])]}[sys.argv[4]]
np.savez(sys.argv[3], *fn())
"""


def run_ref(tmp, what, **arrays):
    """One call of the reference's C++ in a fresh process -> its outputs, in order."""
    src, dst = os.path.join(tmp, "in.npz"), os.path.join(tmp, "out.npz")
    np.savez(src, **arrays)
    subprocess.check_call([sys.executable, "-c", _CHILD, REFDIR, src, dst, what])
    z = np.load(dst)
    return [z["arr_%d" % i] for i in range(len(z.files))]


def like(r, o):
    """The reference's output in the dtype / shape the restatement returns (must be lossless)."""
    c = np.asarray(r).astype(o.dtype).reshape(o.shape)
    assert np.array_equal(c, np.asarray(r).reshape(o.shape), equal_nan=c.dtype.kind == "f"), "lossy conversion"
    return c


def ins(**arrays):
    return {k: T.sha(v) for k, v in arrays.items()}


def main():
    assert os.path.exists(os.path.join(REFDIR, ".built")), "build oracle/_ref first: make -C oracle ref"
    out = {"numpy": np.__version__, "glibc": os.confstr("CS_GNU_LIBC_VERSION")}
    with tempfile.TemporaryDirectory(prefix="rpcc_golden_cpp_") as tmp:
        xyz = T._project_inputs()
        out["project"] = {}
        for geom in sorted(orc.GEOMS):
            g = orc.LidarGeom(**orc.GEOMS[geom])
            geom_v = np.array([g.H, g.W, g.horizontal_FOV, g.vertical_max, g.vertical_min], np.float64)
            ri_r, = run_ref(tmp, "project", xyz=xyz, geom=geom_v)
            out["project"][geom] = {"in": ins(xyz=xyz), "ri": T.sha(like(ri_r, orc.project(xyz, g)))}

        seg, ri, tm = T._point_modeling_inputs()
        pm_r, = run_ref(tmp, "point_modeling", seg=seg, ri=ri)
        pm_r = like(pm_r, orc.point_modeling(ri, seg))
        mp = T._model_param(pm_r)
        pr_r, = run_ref(tmp, "intra_predict", seg=seg, mp=mp, tm=tm)
        out["point_modeling"] = {"in": ins(seg=seg, ri=ri, mp=mp), "pm": T.sha(pm_r),
                                 "pred": T.sha(like(pr_r, orc.intra_predict(seg, mp, tm)))}

        seg, res, kp = T._quantizer_inputs()
        lk, la = T.QUANT_LEVELS
        q_r, = run_ref(tmp, "uniform_quantize", seg=seg, res=res)
        qn_r, s_r = run_ref(tmp, "nonuniform_quantize", seg=seg, res=res, kp=kp, lk=lk, la=la)
        qn_o, s_o = orc.nonuniform_quantize(seg, res, kp, lk, la, 2)
        out["quantizers"] = {"in": ins(seg=seg, res=res, kp=kp), "q": T.sha(like(q_r, orc.uniform_quantize(seg, res, 0.04))),
                             "qn": T.sha(like(qn_r, qn_o)), "sal": T.sha(like(s_r, s_o))}

        # the hostile values of tests/value_cases.py: Table A through both quantisers, scene B through the predictor and both quantisers
        seg, res, kp = T._value_table_inputs()
        lkv, lav = np.array(T.vc.LEVEL_KP_NUM), T.vc.LABEL_STEPS
        qn_r, s_r = run_ref(tmp, "nonuniform_quantize", seg=seg, res=res, kp=kp, lk=lkv, la=lav, gl=np.array(T.vc.GROUND_LEVEL))
        qn_o, s_o = orc.nonuniform_quantize(seg, res, kp, lkv, lav, T.vc.GROUND_LEVEL)
        out["value_table"] = {"in": ins(seg=seg, res=res, kp=kp), "q": {}, "qn": T.sha(like(qn_r, qn_o)), "sal": T.sha(like(s_r, s_o))}
        for step in T.vc.UNIFORM_STEPS:
            q_r, = run_ref(tmp, "uniform_quantize", seg=seg, res=res, acc=np.array(float(step)))
            out["value_table"]["q"][T._step_key(step)] = T.sha(like(q_r, orc.uniform_quantize(seg, res, float(step))))
        out["scene_b"] = {}
        for frame in (0, 1):
            seg, mp, tm, ri, kp = T._scene_b_inputs(frame)
            pr_r, = run_ref(tmp, "intra_predict", seg=seg, mp=mp, tm=tm)
            pr_r = np.asarray(pr_r, np.float32).reshape(seg.shape + (1,))
            with np.errstate(all="ignore"):
                res = (ri - pr_r[..., 0]).astype(np.float32)
            q_r, = run_ref(tmp, "uniform_quantize", seg=seg, res=res)
            qn_r, s_r = run_ref(tmp, "nonuniform_quantize", seg=seg, res=res, kp=kp, lk=lk, la=la)
            qn_o, s_o = orc.nonuniform_quantize(seg, res, kp, lk, la, 2)
            out["scene_b"][str(frame)] = {"in": ins(seg=seg, mp=mp, tm=tm, ri=ri, kp=kp, res=T._nan_canon(res)), "pred": T.sha(T._nan_canon(pr_r)),
                                          "q": T.sha(like(q_r, orc.uniform_quantize(seg, res, 0.04))), "qn": T.sha(like(qn_r, qn_o)),
                                          "sal": T.sha(like(s_r, s_o))}

        # the cells compared are the ones the restatement writes (feat != 0; key points > 0), as the test selects them
        seg, ri = T._feature_inputs()
        f_r, k_r = run_ref(tmp, "features", seg=seg, ri=ri, params=np.array([3, 8, 4, 8, 6]))
        f_o, k_o = orc.extract_features_with_segment(ri, seg)
        f_r, k_r = like(f_r, f_o), like(k_r, k_o)
        out["features"] = {"in": ins(seg=seg, ri=ri), "f_written": T.sha(f_r[f_o != 0]), "k_written": T.sha(k_r[k_o > 0])}

        out["feature_sweep"] = {}
        for params in T.FEATURE_PARAM_DRAWS:
            seg, ri = T._feature_sweep_inputs(params)
            f_r, k_r = run_ref(tmp, "features", seg=seg, ri=ri, params=np.array(params))
            f_o, k_o = orc.extract_features_with_segment(ri, seg, *params)
            f_r, k_r = like(f_r, f_o), like(k_r, k_o)
            out["feature_sweep"][",".join(str(v) for v in params)] = {"in": ins(seg=seg, ri=ri), "f_written": T.sha(f_r[f_o != 0]),
                                                                      "k": T.sha(k_r)}

        out["feature_classes"] = {}
        for W, params in T.fc.FEATURE_PIN_DRAWS:
            seg, ri = T._feature_class_inputs(W, params)
            f_r, k_r = run_ref(tmp, "features", seg=seg, ri=ri, params=np.array(params))
            f_o, k_o = orc.extract_features_with_segment(ri, seg, *params)
            f_r, k_r = like(f_r, f_o), like(k_r, k_o)
            out["feature_classes"]["%d:%s" % (W, ",".join(str(v) for v in params))] = {"in": ins(seg=seg, ri=ri), "f_written": T.sha(f_r[f_o != 0]),
                                                                                      "k": T.sha(k_r)}

        seg = T._contour_inputs()
        cm_r, sq_r = run_ref(tmp, "contour", seg=seg)
        cm_o, sq_o = orc.extract_contour(seg)
        rec_r, = run_ref(tmp, "recover_map", cm=cm_r, sq=sq_r)
        out["contour"] = {"in": ins(seg=seg), "cm": T.sha(like(cm_r, cm_o)), "sq": T.sha(like(sq_r, sq_o)),
                          "recovered": T.sha(like(rec_r, orc.recover_map(cm_o, sq_o)))}
    json.dump(out, open(os.path.join(HERE, "ref_cpp_manifest.json"), "w"), indent=1, sort_keys=True)
    print("wrote", os.path.join(HERE, "ref_cpp_manifest.json"))


if __name__ == "__main__":
    main()
