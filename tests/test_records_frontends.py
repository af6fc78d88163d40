"""The front ends of the NCLT record format that need no GPU: NcltDataset, build_dataset's point_format and registry entry, the tools'
--input_format flag and its argument errors, and the refusals by name."""
import os

import numpy as np
import pytest

import records_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(HERE, "golden", "nclt_records_32E.npz")) as z:
        return z["records"], z["rows"]


def test_nclt_dataset_reads_a_record_file(tmp_path, golden):
    import rpcc_amd  # noqa: F401
    from rpcc_amd.dataset import DatasetTemplate, NcltDataset, build_dataset
    recs, rows = golden
    path = str(tmp_path / "1357847238732390.bin")
    recs.tofile(path)
    lst = tmp_path / "list.txt"
    lst.write_text(path + "\n")
    ds = build_dataset(datalist=str(lst), point_format="nclt")
    assert isinstance(ds, NcltDataset) and isinstance(ds, DatasetTemplate) and len(ds) == 1
    xyz = ds.load_data(path)
    assert xyz.dtype == np.float32 and xyz.shape == (recs.shape[0], 3)
    assert np.array_equal(xyz.view(np.uint32), np.ascontiguousarray(rows[:, :3]).view(np.uint32))      # the reference's preprocessing, bit for bit
    full = ds.load_rows(path)
    assert full.dtype == np.float32 and full.shape == (recs.shape[0], 4)
    assert np.array_equal(full, R.unpack_ref(recs)) and np.array_equal(full[:, 3], recs[:, 6])
    # the float reader on the same name reads something else: the format is the class, not the file name
    plain = build_dataset(datalist=str(lst))
    assert type(plain) is DatasetTemplate
    even = str(tmp_path / "even.bin")
    recs[:3000].tofile(even)
    assert plain.load_data(even).shape == (1500, 3) and ds.load_data(even).shape == (3000, 3)
    with pytest.raises(ValueError, match="point_format"):
        build_dataset(point_format="kitti")
    bad = tmp_path / "short.bin"
    bad.write_bytes(b"\0" * 12)
    with pytest.raises(ValueError, match="no whole number"):
        ds.load_rows(str(bad))


def test_registry_entry():
    import rpcc_amd  # noqa: F401
    from rpcc_amd import dataset as D
    assert D.__dataset_cfg__["NCLT_sync"] == D.__dataset_cfg__["NCLT"] == D.__lidar_cfg__["Velodyne32E"]
    assert D.__dataset_point_format__ == {"NCLT_sync": "nclt"}      # "NCLT" keeps reading preprocessed float files


def test_input_format_flag_on_all_four_tools():
    import rpcc_amd  # noqa: F401
    from rpcc_amd.tools.compress import make_parser, point_format_of
    for datalist in (False, True):      # compress.py / decompress.py share one parser, the datalist tools the other
        p = make_parser(datalist=datalist)
        assert p.parse_args([]).input_format == "float" and point_format_of(p.parse_args([])) is None
        a = p.parse_args(["--input_format", "nclt"])
        assert a.input_format == "nclt" and point_format_of(a) == "nclt"
        with pytest.raises(SystemExit):
            p.parse_args(["--input_format", "pcd"])
    import rpcc_amd.tools.compress_datalist as cd
    import rpcc_amd.tools.decompress as de
    import rpcc_amd.tools.decompress_datalist as dd
    assert cd.point_format_of is de.point_format_of is dd.point_format_of is point_format_of


@pytest.mark.parametrize("ingest", ("rows", "xyz"))
def test_input_format_nclt_excludes_ingest(tmp_path, ingest):
    import rpcc_amd  # noqa: F401
    from rpcc_amd.tools import compress_datalist as cd
    from rpcc_amd.tools.compress import make_parser
    lst = tmp_path / "list.txt"
    lst.write_text("a.bin\n")
    args = make_parser(datalist=True).parse_args(["--datalist", str(lst), "--output_dir", str(tmp_path), "--lidar", "Velodyne32E",
                                                  "--input_format", "nclt", "--ingest", ingest])
    with pytest.raises(SystemExit, match="--input_format nclt .* does not go with --ingest %s" % ingest):
        cd.compress(args, streaming_factory=lambda *a, **k: pytest.fail("nothing may be built"))
    with pytest.raises(SystemExit, match="does not go with"):
        cd.resolve_ingest(ingest, ["a.bin"], point_format="nclt")


def test_resolve_ingest_keeps_the_float_rules():
    import rpcc_amd  # noqa: F401
    from rpcc_amd.tools.compress_datalist import resolve_ingest
    assert resolve_ingest("auto", ["a.bin", "b.bin"], point_format="nclt") == "nclt"
    assert resolve_ingest("auto", ["a.bin"], intensity=True, point_format="nclt") == "nclt"
    assert resolve_ingest("auto", ["a.bin", "b.bin"]) == "rows"
    assert resolve_ingest("auto", ["a.bin", "b.npy"]) == "xyz"
    assert resolve_ingest("xyz", ["a.bin"]) == "xyz"
    assert resolve_ingest("auto", []) == "xyz"
    assert resolve_ingest("auto", ["a.bin"], intensity=True) == "rows"
    for kw in (dict(want="rows", names=["a.npy"]), dict(want="xyz", names=["a.bin"], intensity=True), dict(want="auto", names=["a.npy"], intensity=True)):
        with pytest.raises(SystemExit):
            resolve_ingest(**kw)


def test_refusals_by_name():
    import rpcc_amd  # noqa: F401
    from rpcc_amd import records
    from rpcc_amd.pipeline import MixedBatchCompressor
    with pytest.raises(NotImplementedError, match="MixedBatchCompressor: point_format 'nclt'"):
        MixedBatchCompressor({}, point_format="nclt")
    with pytest.raises(ValueError, match="point_format"):
        records.check_point_format("rows")
    assert records.check_point_format(None) is None and records.check_point_format("nclt") == "nclt"
