#!/usr/bin/env python3
"""Writes tests/golden/nclt_records_32E.npz by running the GENUINE reference's NcltDataset (needs the reference checkout and the module
stubs of gen_golden.py): a few thousand NCLT velodyne_sync records -- a synthetic HDL-32E sweep quantised to records
(tests/records_ref.py: synthetic_records), plus records that hold 0, 19999, 20000, 20001 and 65535 in each field -- are written to a
record file, read back with load_original_utf8_data (dataset/datasets/nclt_dataset.py:36-63) and put through the cast of
preprocess_original_utf8_to_bin_file (:31-33).  The fixture stores the record bytes and the float32 rows the reference produced:
data only.  The reference writes 0 in the fourth column; so does the fixture.

Run from the repository root: python tests/golden/gen_golden_nclt.py"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import gen_golden as G  # noqa: E402
import records_ref as R  # noqa: E402

SWEEP = dict(frame_id=7, H=32, W=128)


def edge_records():
    """Every combination of the edge values over the three fields, intensities and laser bytes running."""
    e = np.array(R.EDGE_VALUES, dtype=np.int64)
    x, y, z = (a.reshape(-1) for a in np.meshgrid(e, e, e, indexing="ij"))
    n = x.shape[0]
    r = np.zeros((n, R.RECORD_BYTES), np.uint8)
    r[:, :6] = np.stack([x, y, z], 1).astype("<u2").view(np.uint8).reshape(n, 6)
    r[:, 6] = (np.arange(n) * 2 + 1) % 256
    r[:, 7] = np.arange(n) % 32
    return r


def main():
    G.install_stubs()
    from dataset.datasets.nclt_dataset import NcltDataset
    recs = np.concatenate([R.synthetic_records(**SWEEP), edge_records()])
    ds = NcltDataset()
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "1357847238732390.bin")
        recs.tofile(path)
        point_cloud = ds.load_original_utf8_data(path)
    point_cloud = np.append(point_cloud, np.zeros((point_cloud.shape[0], 1)), axis=1)       # nclt_dataset.py:32
    rows = point_cloud.astype(np.float32)                                                   # nclt_dataset.py:33
    assert rows.shape == (recs.shape[0], 4)
    np.savez_compressed(os.path.join(HERE, "nclt_records_32E.npz"), records=recs, rows=rows)
    print("%d records (%d of the sweep, %d edge records)" % (recs.shape[0], recs.shape[0] - len(R.EDGE_VALUES) ** 3, len(R.EDGE_VALUES) ** 3))


if __name__ == "__main__":
    main()
