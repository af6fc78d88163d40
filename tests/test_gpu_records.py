"""librpcc_records.so on the GPU: records.unpack bit-equal to tests/records_ref.py on every field value, at the sizes where the launch
takes another path (the head and tail records around the 16-byte pairs, a base that is 8 but not 16 bytes aligned, the capped grid's second
trip), inside guard bytes, and behind every front end: BatchCompressor(point_format="nclt"), StreamingCompressor(ingest="nclt") and
tools/compress.py --input_format nclt write the containers of the float rows the reference's preprocessing makes of the same records."""
import os

import numpy as np
import pytest
import torch

import buffer_arena as BA
import records_caps as RC
import records_ref as R

pytestmark = pytest.mark.gpu

GEOM = "Velodyne32E"
M, ACC = 20, 0.02


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as ge
    ge.build()
    from rpcc_amd import records
    assert torch.cuda.is_available()
    return dict(records=records, dev=torch.device("cuda:0"))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def run(env, recs, shift=0):
    """recs uint8 [N,8] -> the rows records.unpack gives, from a buffer that starts `shift` records into its allocation."""
    host = np.concatenate([np.full((shift, 8), 0xEE, np.uint8), recs]) if shift else recs
    dev = torch.from_numpy(np.ascontiguousarray(host)).to(env["dev"])
    view = dev[shift:]
    assert view.numel() == 0 or view.data_ptr() == dev.data_ptr() + 8 * shift
    rows = env["records"].unpack(view)
    torch.cuda.synchronize()
    assert rows.dtype == torch.float32 and tuple(rows.shape) == (recs.shape[0], 4)
    return rows.cpu().numpy()


@pytest.fixture(scope="module")
def sweeps():
    recs = np.concatenate([R.field_sweep(f) for f in range(3)])
    return recs, R.unpack_ref(recs)


def test_every_field_value(env, sweeps):
    recs, want = sweeps
    got = run(env, recs)
    assert np.array_equal(bits(got), bits(want))
    assert bits(got)[20000, 0] == 0 and bits(got)[65536 + 20000, 1] == 0 and bits(got)[2 * 65536 + 20000, 2] == 0     # +0.0 at the origin
    assert set(got[:, 3].tolist()) == set(float(i) for i in range(256))
    assert np.array_equal(bits(run(env, recs.reshape(-1).reshape(-1, 8))), bits(want))
    flat = env["records"].unpack(torch.from_numpy(recs.reshape(-1)).to(env["dev"]))      # a flat tensor is the same records
    assert np.array_equal(bits(flat.cpu().numpy()), bits(want))


@pytest.mark.parametrize("shift", (0, 1), ids=("aligned", "one-record-in"))
@pytest.mark.parametrize("total", (0, 1, 2, 63, 64, 65, 4097))
def test_small_counts_and_a_base_one_record_in(env, sweeps, total, shift):
    """Aligned: no head record, a tail record when total is odd.  One record in (8 but not 16 bytes aligned): a head record, and a tail
    record when total is even."""
    recs, want = sweeps
    lo = 19990       # around the origin value of the x field
    got = run(env, recs[lo: lo + total], shift=shift)
    assert np.array_equal(bits(got), bits(want[lo: lo + total])), (total, shift)


@pytest.mark.parametrize("shift", (0, 1), ids=("aligned", "one-record-in"))
def test_past_the_grid_cap(env, shift):
    total = RC.past_the_cap_total()
    npairs = (total - shift) // 2
    assert RC.grid(npairs) == RC.REC_GRID_CAP and RC.trips(npairs) == 2
    assert 0 < npairs - RC.PAIRS_PER_TRIP < RC.PAIRS_PER_TRIP and (npairs - RC.PAIRS_PER_TRIP) % 64      # a partial second trip, a partial wavefront
    assert shift + 2 * npairs == total - (1 - shift)       # aligned: a tail record; one record in: a head record and no tail
    assert 8 * total < 32 << 20
    rng = np.random.default_rng(5)
    recs = rng.integers(0, 256, (total, 8), dtype=np.uint8)
    recs[-3:, :6] = np.array([20000, 0, 65535], "<u2").view(np.uint8)     # the last rows are not zero rows by accident
    got = run(env, recs, shift=shift)
    assert np.array_equal(bits(got), bits(R.unpack_ref(recs)))


@pytest.mark.parametrize("shift", (0, 1), ids=("aligned", "one-record-in"))
@pytest.mark.parametrize("total", (1, 1000, 1001))
def test_output_between_guards(env, sweeps, total, shift):
    """rows of exactly total * 16 bytes between guard bytes, pre-filled with NaN words: every row is written, nothing else is."""
    recs, want = sweeps
    lo = 65536 + 19000
    src = torch.from_numpy(np.concatenate([np.zeros((shift, 8), np.uint8), recs[lo: lo + total]])).to(env["dev"])[shift:]
    arena = BA.Arena(16 * total, device=env["dev"], front=4096, back=1 << 16).fill("nan")
    out = arena.view.view(torch.float32).view(total, 4)
    assert torch.isnan(out).all()
    res = env["records"].unpack(src, out=out)
    torch.cuda.synchronize()
    assert res.data_ptr() == arena.view.data_ptr()
    assert arena.check_guards() is None
    assert np.array_equal(bits(out.cpu().numpy()), bits(want[lo: lo + total]))
    with pytest.raises(ValueError, match="out must be"):
        env["records"].unpack(src, out=torch.empty((total + 1, 4), dtype=torch.float32, device=env["dev"]))


# ---- front ends ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def e2e(env):
    from rpcc_amd import dataset, pipeline
    T = dataset.build_dataset(lidar_type=GEOM).PCTransformer
    recs = [R.synthetic_records(9300 + i) for i in range(3)]
    return dict(env, pl=pipeline, T=T, recs=recs, rows=[R.unpack_ref(r) for r in recs])


def mk(e2e, **kw):
    return e2e["pl"].BatchCompressor(e2e["T"], cluster_num=M, accuracy=ACC, basic_compressor="bzip2", seed=4, **kw)


@pytest.mark.parametrize("scale", (None, 1.0), ids=("geometry", "intensity_scale=1"))
def test_batch_compressor(e2e, scale):
    from rpcc_amd import compress_utils as cu
    from rpcc_amd import ops
    from rpcc_amd.tools.decompress import decode_frame
    T, dev = e2e["T"], e2e["dev"]
    recs = [e2e["recs"][0], np.zeros((0, 8), np.uint8), e2e["recs"][1]]
    rows = [e2e["rows"][0], np.zeros((0, 4), np.float32), e2e["rows"][1]]
    got = mk(e2e, point_format="nclt", intensity_scale=scale).compress(recs, frame_ids=[3, 4, 5])
    want = mk(e2e, intensity_scale=scale).compress(rows if scale is not None else [r[:, :3] for r in rows], frame_ids=[3, 4, 5])
    assert len(got) == 3 and got == want
    assert mk(e2e, point_format="nclt", intensity_scale=scale).compress([r.reshape(-1) for r in recs], frame_ids=[3, 4, 5]) == want     # flat arrays
    if scale is None:
        return
    host = cu.BasicCompressor(method_name="bzip2")
    for b in (0, 2):
        _, _, seg, w = decode_frame(cu.unpack_bitstream(got[b], intensity=True), host, T, M, 2 * ACC, None, True, want_points=False, intensity=True)
        # every owner pixel's record byte: the owners by the intensity kernels on the reference rows and the image the rows project to
        rows_d = torch.from_numpy(rows[b]).to(dev)
        offs = torch.tensor([0, rows_d.shape[0]], dtype=torch.int64, device=dev)
        ri = ops.project(rows_d, offs, T.geom)
        own = torch.empty_like(ri)
        ops.intensity_encode(rows_d, offs, T.geom, ri, 1.0, owner_intensity=own)
        set_ = (ri != 0)[0].cpu().numpy()
        assert set_.sum() > 10000 and np.array_equal(seg != 1, set_)
        assert np.array_equal(w[set_], own[0].cpu().numpy()[set_])
        assert np.array_equal(w[set_], np.rint(w[set_])) and w[set_].max() <= 255 and len(np.unique(w[set_])) > 100     # bytes, losslessly
        assert not w[~set_].any()


def test_streaming_loader(e2e, tmp_path):
    """Record files through ingest="nclt" against ingest="rows" on the float files the reference's preprocessing writes of them (fourth
    column 0): two batches, the last one short, and slots sized too small, so that they grow."""
    from rpcc_amd.loader import StreamingCompressor
    rec_paths, row_paths = [], []
    for i, (r, rows) in enumerate(zip(e2e["recs"], e2e["rows"])):
        rec_paths.append(str(tmp_path / ("sync_%d.bin" % i)))
        r.tofile(rec_paths[-1])
        pre = rows.copy()
        pre[:, 3] = 0
        row_paths.append(str(tmp_path / ("pre_%d.bin" % i)))
        pre.tofile(row_paths[-1])
    fids = [[11, 12], [13]]

    def stream(ingest, paths, **kw):
        got = {}
        sc = StreamingCompressor(mk(e2e, **kw), batch=2, depth=2, workers=2, ingest=ingest, points_per_frame=1000)
        assert sc.run([(paths[:2], fids[0]), (paths[2:], fids[1])], sink=lambda k, blobs: got.update({k: blobs})) == 3
        assert sc.grown >= 1
        return got[0] + got[1], sc

    want, _ = stream("rows", row_paths)
    got, sc = stream("nclt", rec_paths)
    assert len(got) == 3 and got == want
    assert all(s.xyz_pin is None and s.rec_pin.shape == (s.cap, 8) and s.rec_dev.shape == (s.cap, 8) and s.xyz_dev.shape == (s.cap, 4) for s in sc.slots)
    assert want[:2] == mk(e2e).compress([r[:, :3] for r in e2e["rows"][:2]], frame_ids=fids[0])     # and both are the batch compressor's
    # arrays in the place of paths, and the intensity payload from the records' bytes
    inten_want = mk(e2e, intensity_scale=1.0).compress(e2e["rows"][:2], frame_ids=fids[0])
    got = {}
    sc = StreamingCompressor(mk(e2e, intensity_scale=1.0), batch=2, depth=2, workers=2, ingest="nclt")
    assert sc.run([([rec_paths[0], e2e["recs"][1]], fids[0])], sink=lambda k, blobs: got.update({k: blobs})) == 2
    assert got[0] == inten_want and sc.grown == 0
    bad = tmp_path / "short.bin"
    bad.write_bytes(b"\0" * 12)
    with pytest.raises(ValueError, match="no whole number of 8-byte NCLT records"):
        sc.run([([str(bad)], [0])])


def test_compress_tool(e2e, tmp_path, capsys):
    from rpcc_amd.tools import compress as tc
    src, pre = tmp_path / "1357847238732390.bin", tmp_path / "0000000000.bin"
    e2e["recs"][2].tofile(src)
    rows = e2e["rows"][2].copy()
    rows[:, 3] = 0                       # preprocess_original_utf8_to_bin_file
    rows.tofile(pre)
    base = ["--lidar", GEOM, "--basic_compressor", "bzip2", "--cluster_num", str(M)]
    out, ref = tmp_path / "sync.rpcc", tmp_path / "pre.rpcc"
    # (the seeded fits draw with the frame's identity, which comes from the file name: both runs read files of one name in turn)
    tc.compress(tc.make_parser().parse_args(["--input", str(pre), "--output", str(ref)] + base))
    os.replace(pre, tmp_path / "kept.bin")
    os.replace(src, pre)
    tc.compress(tc.make_parser().parse_args(["--input", str(pre), "--output", str(out), "--input_format", "nclt"] + base))
    capsys.readouterr()
    assert os.path.getsize(out) > 1000 and open(out, "rb").read() == open(ref, "rb").read()
    # the way back: --input_format says how --original_point_cloud is read; both originals give the same comparison
    from rpcc_amd.tools import decompress as td
    texts = []
    for orig, fmt in ((pre, ["--input_format", "nclt"]), (tmp_path / "kept.bin", [])):
        td.decompress(td.make_parser().parse_args(["--input", str(out), "--output", str(tmp_path / "rec.bin"), "--eval", "--original_point_cloud", str(orig)]
                                                  + fmt + base))
        text = capsys.readouterr().out
        texts.append(text[text.index("    BPP: "):])
    assert "Depth Error (max): " in texts[0] and texts[0] == texts[1]


def test_compress_datalist_tool(e2e, tmp_path):
    """tools/compress_datalist.py --input_format nclt (ingest "nclt", paths read in place): the files of the batch compressor fed the float rows."""
    from rpcc_amd.tools import compress_datalist as cd
    from rpcc_amd.tools.compress import make_parser
    from rpcc_amd.utils import frame_identity
    names = []
    for i, r in enumerate(e2e["recs"]):
        names.append(str(tmp_path / "in" / ("%d.bin" % (1357847238732390 + i))))
        os.makedirs(os.path.dirname(names[-1]), exist_ok=True)
        r.tofile(names[-1])
    lst = tmp_path / "list.txt"
    lst.write_text("".join(n + "\n" for n in names))
    out = tmp_path / "out"
    cd.compress(make_parser(datalist=True).parse_args(["--datalist", str(lst), "--output_dir", str(out), "--lidar", GEOM, "--basic_compressor", "bzip2",
                                                       "--cluster_num", str(M), "--seed", "4", "--batch", "2", "--workers", "2", "--input_format", "nclt"]))
    want = mk(e2e).compress([r[:, :3] for r in e2e["rows"]], frame_ids=[frame_identity(n) for n in names])
    for n, blob in zip(names, want):
        assert open(cd.output_path_for(str(out), n), "rb").read() == blob, n
