"""CPU: what the device entropy back-ends share on the host.  BasicCompressor's resolution of (method, flags) to a back-end, against the
table written out below, and rpcc_amd.entropy's slot layouts against the expressions the codec modules used before they shared them."""
import bz2
import gzip
import itertools

import numpy as np
import pytest

METHODS = ("lz4", "bzip2", "gzip", "deflate")


def _has_lz4():
    try:
        import lz4  # noqa: F401
        return True
    except ImportError:
        return False


def _expected(method, entropy, bunzip2, bzip2):
    """((module, function) of batch_codec() or None, (module, function) of batch_decoder() or None) -- the table, as a literal."""
    if method == "lz4":
        return ("lz4_codec", "dumps_many"), ("lz4_codec", "loads_many")
    if method == "bzip2":
        return (("bzip2_codec", "compress_many") if bzip2 else None), (("bunzip2_codec", "decompress_many") if bunzip2 else None)
    return (("deflate_codec", "compress_many"), ("inflate_codec", "decompress_many")) if entropy else (None, None)


def _name(f):
    return None if f is None else (f.__module__.rsplit(".", 1)[-1], f.__name__)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("flags", list(itertools.product((False, True), repeat=3)), ids=lambda f: "".join("01"[b] for b in f))
def test_resolution_table(method, flags):
    import rpcc_amd  # noqa: F401
    from rpcc_amd import compress_utils as cu
    if method == "lz4" and _has_lz4():
        pytest.skip("the lz4 package is installed: 'lz4' runs through it and has no list coder")
    entropy, bunzip2, bzip2 = flags
    bc = cu.BasicCompressor(method_name=method, device_entropy=entropy, device_bunzip2=bunzip2, device_bzip2=bzip2)
    codec, decoder = _expected(method, entropy, bunzip2, bzip2)
    got = bc.batch_codec()
    assert (None if got is None else (got[0].__name__.rsplit(".", 1)[-1], _name(got[1]))) == (None if codec is None else (codec[0], codec))
    assert _name(bc.batch_decoder()) == decoder
    assert bc.lz4_batched() is (method == "lz4")
    assert bool(bc.deflate_batched()) is (method in ("gzip", "deflate") and entropy)
    assert bool(bc.bzip2_batched()) is (method == "bzip2" and bzip2)


def test_no_flag_is_the_stdlib():
    import rpcc_amd  # noqa: F401
    from rpcc_amd import compress_utils as cu
    a = np.arange(5000, dtype=np.int16) % 37
    for method, lib in (("bzip2", bz2), ("gzip", gzip), ("deflate", gzip)):
        bc = cu.BasicCompressor(method_name=method)
        blob = bc.compress(a)
        assert lib.decompress(blob) == a.tobytes()
        if lib is bz2:
            assert blob == bz2.compress(a)
        else:
            assert blob[:4] == gzip.compress(a)[:4] and blob[8:] == gzip.compress(a)[8:]      # bytes 4..7: the time of the call
        assert bc.decompress(lib.compress(a)) == a.tobytes()
        assert bc.compress_dict({"x": a}).keys() == {"x"} and bc.decompress_dict({"x": lib.compress(a)}) == {"x": a.tobytes()}
        assert bc.decompress_dicts([{"x": lib.compress(a)}, {"y": lib.compress(b"")}]) == [{"x": a.tobytes()}, {"y": b""}]
    with pytest.raises(ValueError, match="no compression method set"):
        cu.BasicCompressor().compress(a)
    with pytest.raises(ValueError, match="no compression method set"):
        cu.BasicCompressor().decompress(b"")
    assert cu.BasicCompressor().batch_codec() is None and cu.BasicCompressor().batch_decoder() is None


SIZES = ([], [0], [1], [7, 8, 9], [0, 0, 5], [4097])


@pytest.mark.parametrize("sizes", SIZES, ids=str)
def test_packed_slots(sizes):
    """The encoders' layout: back to back, no padding (lz4_codec.pack_containers reads the slots that way)."""
    import rpcc_amd  # noqa: F401
    from rpcc_amd import entropy
    cap = np.array(sizes, np.int64)
    off, total = entropy.packed_slots(sizes)
    want = np.zeros(len(cap), np.int64)        # the encoders' expressions before the layout was shared
    want[1:] = np.cumsum(cap)[:-1]
    assert off.dtype == np.int64 and off.tolist() == want.tolist() and total == int(cap.sum())
    assert (np.diff(off) >= 0).all() and (off[1:] == off[:-1] + cap[:-1]).all()
    assert isinstance(total, int)


@pytest.mark.parametrize("sizes", SIZES, ids=str)
def test_aligned_slots(sizes):
    """The decoders' layout and the staged inputs': every slot at an 8-byte multiple, the last one not rounded up."""
    import rpcc_amd  # noqa: F401
    from rpcc_amd import entropy
    cap = np.array(sizes, np.int64)
    off, end = entropy.aligned_slots(sizes)
    want = np.zeros(len(cap), np.int64)        # the decoders' expressions before the layout was shared
    want[1:] = np.cumsum((cap + 7) // 8 * 8)[:-1]
    assert off.dtype == np.int64 and off.tolist() == want.tolist()
    assert end == (int(want[-1] + cap[-1]) if len(cap) else 0) and isinstance(end, int)
    assert (off % 8 == 0).all() and (np.diff(off) >= 0).all() and (off[1:] >= off[:-1] + cap[:-1]).all()
    # the staging buffer: the rounded total, as the sum of the rounded sizes was
    assert (end + 7) // 8 * 8 == int(((cap + 7) // 8 * 8).sum())
