"""records.unpack_host and the two statements of tests/records_ref.py against the golden the genuine reference produced
(tests/golden/nclt_records_32E.npz, gen_golden_nclt.py) and against each other on every field value.  No GPU needed."""
import os

import numpy as np
import pytest

import records_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(HERE, "golden", "nclt_records_32E.npz")) as z:
        return z["records"], z["rows"]


@pytest.fixture(scope="module")
def records_mod():
    import rpcc_amd  # noqa: F401
    from rpcc_amd import records
    return records


def test_golden_holds_the_edge_values(golden):
    recs, rows = golden
    assert recs.dtype == np.uint8 and recs.shape[1] == 8 and rows.dtype == np.float32 and rows.shape == (recs.shape[0], 4)
    fields = recs[:, :6].copy().view("<u2")
    for f in range(3):
        assert set(R.EDGE_VALUES) <= set(fields[:, f].tolist())
    assert 2000 < recs.shape[0] < 10000
    assert not rows[:, 3].any()      # the reference's preprocessing writes 0 there


def test_every_statement_equals_the_reference(golden, records_mod):
    recs, rows = golden
    for name, got in (("unpack_host", records_mod.unpack_host(recs)), ("unpack_ref", R.unpack_ref(recs)), ("unpack_loop", R.unpack_loop(recs.tobytes()))):
        assert got.dtype == np.float32 and got.shape == rows.shape, name
        assert np.array_equal(bits(got[:, :3]), bits(rows[:, :3])), name          # bit for bit, the sign of zero included
        assert np.array_equal(got[:, 3], recs[:, 6].astype(np.float32)), name     # the intensity byte, where the reference leaves 0


@pytest.mark.parametrize("field", (0, 1, 2))
def test_statements_agree_on_all_field_values(field, records_mod):
    recs = R.field_sweep(field)
    assert np.array_equal(recs[:, :6].copy().view("<u2")[:, field], np.arange(65536))
    want = R.unpack_ref(recs)
    assert np.array_equal(bits(records_mod.unpack_host(recs)), bits(want))
    assert np.array_equal(bits(R.unpack_loop(recs.tobytes())), bits(want))
    assert np.array_equal(want[:, 3], np.arange(65536) % 256)
    assert np.array_equal(records_mod.unpack_host(recs.reshape(-1)), want)       # a flat array is the same records


def test_origin_is_plus_zero_and_a_fused_rule_misses_it():
    v = np.arange(65536)
    recs = R.field_sweep(0)
    x = R.unpack_ref(recs)[:, 0]
    assert bits(x[20000:20001])[0] == 0              # +0.0: no sign bit, no fraction
    assert R.convert(20000, 20000, 20000) == (0.0, 0.0, 0.0)
    # reach: the contracted rule (one rounding of v * 0.005 - 100) differs from the rule at exactly this value, so the exhaustive cases
    # can tell the two apart -- and only there
    fused = R.fused_model(v)
    differ = np.flatnonzero(bits(fused) != bits(x))
    assert differ.tolist() == [20000]
    assert fused[20000] != 0.0 and abs(float(fused[20000])) < 1e-12
    # fp32-only evaluation is no candidate either
    f32 = v.astype(np.float32) * np.float32(0.005) + np.float32(-100.0)
    assert np.count_nonzero(bits(f32) != bits(x)) > 33000


def test_pack_ref_inverts_the_rule():
    for field in range(3):
        recs = R.field_sweep(field)
        rows = R.unpack_ref(recs)
        assert np.array_equal(R.pack_ref(rows[:, :3], recs[:, 6], recs[:, 7]), recs)


def test_read_records(tmp_path, records_mod, golden):
    recs, _ = golden
    p = tmp_path / "sweep.bin"
    recs.tofile(p)
    got = records_mod.read_records(str(p))
    assert got.dtype == np.uint8 and np.array_equal(got, recs)
    q = tmp_path / "rows.bin"
    q.write_bytes(b"\0" * 12)        # one packed xyz point: no whole number of records
    with pytest.raises(ValueError, match="12 bytes is no whole number"):
        records_mod.read_records(str(q))
    e = tmp_path / "empty.bin"
    e.write_bytes(b"")
    assert records_mod.read_records(str(e)).shape == (0, 8)
    assert records_mod.unpack_host(np.zeros((0, 8), np.uint8)).shape == (0, 4)
    assert records_mod.RECORD_BYTES == R.RECORD_BYTES == 8
    for bad in (np.zeros((3, 4), np.uint8), np.zeros((2, 8), np.int8), np.zeros(7, np.uint8)):
        with pytest.raises(ValueError):
            records_mod.unpack_host(bad)
