"""Writes tests/golden/rans_filter_pins.json: length and sha256 of the stream tests/rans_filter_ref.py gives for a few cases of
tests/rans_filter_cases.py -- the three-chunk walk, alt and half contents at every width and both chunk sizes -- and for the example
sweep's residuals at the default chunk size (tests/test_rans_filter_ref.py holds the reference to it).  Run after a deliberate change of a
rule of DESIGN.md section 19, version 2:
    python tests/golden/gen_rans_filter_pins.py"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import rans_filter_cases as C  # noqa: E402
import rans_filter_ref as F  # noqa: E402


def _pin(s, n, width, chunk_log2):
    return {"input": n, "width": width, "chunk_log2": chunk_log2, "magic": s[:2].decode(), "mode": s[2], "length": len(s),
            "sha256": hashlib.sha256(s).hexdigest()}


def pins():
    out = {}
    for name, (x, width, chunk_log2, filt) in C.valid().items():
        if filt == F.FILTER_DELTA and len(x) == 2 * (1 << chunk_log2) + 1 and name.split("_")[1] in ("walk", "alt", "half"):
            out[name] = _pin(C.reference(name), len(x), width, chunk_log2)
    q = np.load(os.path.join(HERE, "example_64E.npz"))["q_uniform"].astype("<i2").tobytes()
    out["golden_residual_quantized"] = _pin(F.encode(q, 2, filter=F.FILTER_DELTA), len(q), 2, F.DEFAULT_CHUNK_LOG2)
    return out


if __name__ == "__main__":
    with open(os.path.join(HERE, "rans_filter_pins.json"), "w") as f:
        json.dump(pins(), f, indent=1, sort_keys=True)
        f.write("\n")
