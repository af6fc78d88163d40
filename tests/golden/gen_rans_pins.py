"""Writes tests/golden/rans_pins.json: length and sha256 of the stream tests/rans_ref.py gives for every case of tests/rans_cases.py
(tests/test_rans_ref.py holds the reference to it).  Run after a deliberate change of a rule of DESIGN.md section 19:
    python tests/golden/gen_rans_pins.py"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import rans_cases as C  # noqa: E402


def pins():
    out = {}
    for name, (x, width, chunk_log2) in C.everything().items():
        s = C.reference(name)
        out[name] = {"input": len(x), "width": width, "chunk_log2": chunk_log2, "mode": s[2], "length": len(s), "sha256": hashlib.sha256(s).hexdigest()}
    return out


if __name__ == "__main__":
    with open(os.path.join(HERE, "rans_pins.json"), "w") as f:
        json.dump(pins(), f, indent=1, sort_keys=True)
        f.write("\n")
