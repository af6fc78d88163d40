"""Writes tests/golden/bzip2_pins.json: length and sha256 of the stream tests/bzip2_ref.py gives for every case of tests/bzip2_cases.py
(tests/test_bzip2_ref.py holds the reference to it).  Run after a deliberate change of a rule of DESIGN.md section 15:
    python tests/golden/gen_bzip2_pins.py"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import bzip2_cases as C  # noqa: E402
import bzip2_ref as R  # noqa: E402


def pins():
    out = {}
    for name, (x, level) in C.everything().items():
        s = R.compress(x, level)
        out[name] = {"input": len(x), "level": level, "length": len(s), "sha256": hashlib.sha256(s).hexdigest()}
    return out


if __name__ == "__main__":
    with open(os.path.join(HERE, "bzip2_pins.json"), "w") as f:
        json.dump(pins(), f, indent=1, sort_keys=True)
        f.write("\n")
