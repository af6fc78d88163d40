"""Generates tests/golden/lz4_foreign.npz: the arrays of the example sweep (example_64E.npz; contour bits, index sequence and
models as oracle.pack_payload builds them, both residual arrays) compressed by the system liblz4 (LZ4_compress_default), in
python-lz4 0.7.0's dumps form (uint32 LE size + block).  These are streams of a parse other than the build's own, so the GPU
decoder is checked against foreign input where liblz4 is not installed.

    python tests/golden/gen_golden_lz4.py        (needs liblz4.so.1; run from the repository root)"""
import ctypes
import os
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def arrays():
    """name -> the uncompressed bytes, in a fixed order."""
    from oracle import oracle as orc
    z = np.load(os.path.join(HERE, "example_64E.npz"))
    od = orc.pack_payload(z["model_param"], z["seg_idx"], None, z["q_uniform"])
    return {"contour_map": od["contour_map"].tobytes(), "idx_sequence": od["idx_sequence"].tobytes(),
            "plane_param": od["plane_param"].tobytes(), "q_uniform": z["q_uniform"].tobytes(), "q_nonuniform": z["q_nonuniform"].tobytes(),
            "zeros": bytes(300000)}


def main():
    lz = ctypes.CDLL("liblz4.so.1")
    out = {}
    for k, src in arrays().items():
        dst = ctypes.create_string_buffer(lz.LZ4_compressBound(len(src)))
        n = lz.LZ4_compress_default(src, dst, len(src), len(dst))
        assert n > 0
        out[k] = np.frombuffer(struct.pack("<I", len(src)) + dst.raw[:n], np.uint8)
        print(k, len(src), n)
    np.savez_compressed(os.path.join(HERE, "lz4_foreign.npz"), **out)


if __name__ == "__main__":
    main()
