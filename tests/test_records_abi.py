"""librpcc_records.so (include/rpcc_records.h) builds, exports what its header declares and refuses bad arguments.  No GPU needed."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    import rpcc_amd  # noqa: F401
    from rpcc_amd import _records_lib
    return _records_lib


def test_header_symbols_exported(built):
    hdr = open(os.path.join(ROOT, "include", "rpcc_records.h")).read()
    declared = sorted(set(re.findall(r"\b(rpcc_[a-z0-9_]+)\s*\(", hdr)))
    assert declared == ["rpcc_records_last_error", "rpcc_records_unpack", "rpcc_records_version"]
    lib = ctypes.CDLL(built.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    assert built.exported_symbols() == declared
    assert int(re.search(r"#define RPCC_RECORDS_ABI_VERSION (\d+)", hdr).group(1)) == built.ABI_VERSION == 1
    for name, val in (("RPCC_RECORDS_BYTES", built.RECORD_BYTES), ("RPCC_RECORDS_MAX_TOTAL", built.MAX_TOTAL)):
        assert int(re.search(r"#define %s \(?(-?\d+)\)?" % name, hdr).group(1)) == val, name
    from rpcc_amd import records
    import records_caps as RC
    import records_ref as R
    assert records.RECORD_BYTES == built.RECORD_BYTES == R.RECORD_BYTES == 8
    assert built.MAX_TOTAL == 2 ** 31 - 1
    assert RC.REC_THREADS % 64 == 0 and RC.REC_GRID_CAP >= 1
    rule = open(os.path.join(ROOT, "r-pcc_amd", "csrc_records", "records_rule.h")).read()
    assert float(re.search(r"#define RECORDS_SCALING ([0-9.]+)", rule).group(1)) == R.SCALING == records.SCALING
    assert float(re.search(r"#define RECORDS_OFFSET \((-[0-9.]+)\)", rule).group(1)) == R.OFFSET == records.OFFSET


def test_version(built):
    assert built.lib().rpcc_records_version() == built.ABI_VERSION


def test_argument_errors_do_not_crash(built):
    lib = built.lib()
    raw = ctypes.create_string_buffer(256 + 64)     # host memory: every call below must refuse before touching it
    base = (ctypes.addressof(raw) + 63) // 64 * 64
    fill = bytes(range(256)) + b"\0" * 64
    ctypes.memmove(raw, fill, len(fill))
    rec, rows = base, base + 64                      # 4 records in [rec, rec + 32), their 4 rows in [rows, rows + 64): no overlap
    call = lambda records=rec, total=4, out=rows: lib.rpcc_records_unpack(records, total, out, None)
    for bad in (dict(total=-1), dict(total=2 ** 31), dict(total=2 ** 40), dict(records=None), dict(out=None), dict(records=None, out=None),
                dict(records=rec + 4), dict(records=rec + 1), dict(out=rows + 8), dict(out=rows + 4),      # misaligned
                dict(records=rows), dict(records=rows + 56), dict(records=rows + 24, total=2), dict(records=rec + 40),   # overlapping
                dict(out=rows + 8, total=0), dict(records=rec + 4, total=0)):          # misaligned at total 0 too
        assert call(**bad) == -1, bad
        assert b"bad argument" in lib.rpcc_records_last_error(), bad
    assert raw.raw == fill


def test_zero_records_is_a_no_op(built):
    lib = built.lib()
    buf = ctypes.create_string_buffer(64)
    base = (ctypes.addressof(buf) + 15) // 16 * 16
    assert lib.rpcc_records_unpack(None, 0, None, None) == 0
    assert lib.rpcc_records_unpack(base, 0, base + 16, None) == 0
    assert lib.rpcc_records_unpack(base, 0, base, None) == 0       # nothing to overlap
    assert buf.raw == b"\0" * 64


def test_source_digest_unchanged_by_the_records_library(built):
    from rpcc_amd import build as b
    before, deps = b.source_digest(), list(b.DEPS)
    b.build_records(force=True)
    assert b.source_digest() == before and b.DEPS == deps
    assert not any("csrc_records" in d or d.endswith("rpcc_records.h") for d in b.DEPS)
    assert os.path.exists(b.RECORDS_LIB)
    here = os.path.dirname(b.__file__)
    assert os.path.join(here, "csrc_records", "records_rule.h") in b.RECORDS_DEPS
    assert os.path.join(here, "csrc_tile", "tiles.h") in b.RECORDS_DEPS      # the shared error state
    assert os.path.join(ROOT, "include", "rpcc_records.h") in b.RECORDS_DEPS


def test_front_ends_name_the_missing_gpu(built):
    """Without a visible GPU records.unpack -- and with it BatchCompressor(point_format="nclt") and StreamingCompressor(ingest="nclt") --
    raises RpccError by name; nothing falls back to the CPU.  A host tensor is refused by name on any machine."""
    import numpy as np
    import torch
    from rpcc_amd import records
    from rpcc_amd._lib import RpccError
    recs = np.zeros((5, 8), np.uint8)
    with pytest.raises(RpccError, match="needs a GPU tensor"):
        records.unpack(torch.from_numpy(recs))
    with pytest.raises(RpccError, match="needs a GPU tensor"):
        records.unpack(recs)
    if torch.cuda.is_available():
        rows = records.unpack(torch.from_numpy(recs).cuda())
        assert rows.shape == (5, 4) and np.array_equal(rows.cpu().numpy(), records.unpack_host(recs))
