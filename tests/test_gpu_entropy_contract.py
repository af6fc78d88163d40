"""-m gpu: one contract over the device entropy back-ends, which share their staging, slot layout and list drivers (rpcc_amd.entropy):
every list encoder's output decodes to its input with the format's host library, and every list decoder returns the bytes of the sound
streams and a status for a truncated one without disturbing its neighbours' slots.  The per-back-end suites hold the detailed checks."""
import bz2
import gzip
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import lz4_ref  # noqa: E402

SIZES = (0, 1, 7, 8, 9, 4097)


@pytest.fixture(scope="module")
def pkg():
    import torch
    assert torch.cuda.is_available()
    import __graft_entry__ as ge
    ge.build()
    import rpcc_amd
    return rpcc_amd


@pytest.fixture(scope="module")
def buffers():
    rng = np.random.default_rng(11)
    # runs and noise, so that the streams hold matches and literals
    return [bytes(np.repeat(rng.integers(0, 256, -(-n // 6), dtype=np.uint8), 6)[:n] ^ (rng.integers(0, 32, n, dtype=np.uint8) == 0)) for n in SIZES]


ENCODERS = {"lz4": ("lz4_codec", "dumps_many", lz4_ref.loads), "deflate": ("deflate_codec", "compress_many", gzip.decompress),
            "bzip2": ("bzip2_codec", "compress_many", bz2.decompress)}
DECODERS = {"lz4": ("lz4_codec", lz4_ref.dumps, lz4_ref.loads), "inflate": ("inflate_codec", gzip.compress, gzip.decompress),
            "bunzip2": ("bunzip2_codec", bz2.compress, bz2.decompress)}


@pytest.mark.parametrize("name", list(ENCODERS))
def test_list_encoders(pkg, buffers, name):
    module, many, host_decode = ENCODERS[name]
    codec = getattr(__import__("rpcc_amd." + module), module)
    blobs = getattr(codec, many)(buffers)
    assert len(blobs) == len(buffers) and all(isinstance(b, bytes) for b in blobs)
    assert [bytes(host_decode(b)) for b in blobs] == buffers
    for k in (0, len(buffers) - 1):                      # a list of one: the empty buffer and the longest
        (one,) = getattr(codec, many)([buffers[k]])
        assert bytes(host_decode(one)) == buffers[k]
    assert getattr(codec, many)([]) == []


@pytest.mark.parametrize("name", list(DECODERS))
def test_list_decoders(pkg, buffers, name):
    module, host_encode, host_decode = DECODERS[name]
    codec = getattr(__import__("rpcc_amd." + module), module)
    streams = [bytes(host_encode(b)) for b in buffers]
    cut = streams[-1][: len(streams[-1]) // 2]
    with pytest.raises((ValueError, OSError, EOFError)):          # the host library refuses it too
        host_decode(cut)
    mixed = streams[:3] + [cut] + streams[3:]
    st, outs = codec.decode_many(mixed)
    assert st.dtype == np.int32 and st[3] != 0 and outs[3] is None
    assert np.delete(st, 3).tolist() == [0] * len(buffers)
    assert outs[:3] + outs[4:] == buffers                          # the bad stream's neighbours among them: the slot offsets are shared
    for k in (0, len(buffers) - 1):
        st, outs = codec.decode_many([streams[k]])
        assert st.tolist() == [0] and outs == [buffers[k]]
    st, outs = codec.decode_many([cut])
    assert st[0] != 0 and outs == [None]
    st, outs = codec.decode_many([])
    assert st.shape == (0,) and outs == []
