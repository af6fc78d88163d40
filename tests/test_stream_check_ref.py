"""The status rule of rpcc_decompress_batch against the table of broken frames (tests/stream_cases.py), the host container parser of
pipeline.BatchDecompressor, and rpcc_decompress_workspace_bytes.  No GPU."""
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_cases as sc  # noqa: E402

GEOMS = ((5, 413, 20), (4, 512, 7))     # (H, W, cluster_num): P % 8 == 1 and three tiles; P a multiple of the tile


@pytest.mark.parametrize("uniform", (True, False))
@pytest.mark.parametrize("H,W,M", GEOMS)
def test_rule_gives_the_table(H, W, M, uniform):
    frames = sc.cases(H, W, M + 2, uniform)
    got = {}
    for f in frames:
        st = sc.stream_status(f["payload"], f["est"], H * W, M + 2, uniform, 4)
        assert st == f["expect"], (f["name"], st, f["expect"])
        got.setdefault(st, []).append(f["name"])
    want = set(range(sc.E_RESIDUAL + 1)) - ({sc.E_SALIENCE} if uniform else set())
    assert set(got) == want, got
    # every second frame is sound, the first and the last too
    assert all(f["expect"] == sc.OK for f in frames[::2]) and len(frames) % 2 == 1
    if (H * W) % 8:
        assert "contour_flip_pad_bit" in got[sc.OK]
    # the frames with two edits pin the order for the codes 2 .. 8: each of them is one of a pair, the earlier check wins
    pairs = [f for f in frames if "+" in f["name"]]
    assert len(pairs) >= (6 if uniform else 8)


def test_codes_match_the_binding_and_the_header():
    import re
    import rpcc_amd  # noqa: F401
    from rpcc_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rpcc_hip.h")).read()
    for name in ("OK", "E_ENTROPY", "E_PLANE", "E_CONTOUR", "E_WIDTH", "E_NSEQ", "E_LABEL", "E_SALIENCE", "E_RESIDUAL", "E_CONTAINER"):
        v = int(re.search(r"#define RPCC_STREAM_%s (\d+)" % name, hdr).group(1))
        assert v == getattr(sc, name) == getattr(_lib, "STREAM_" + name), name
    assert int(re.search(r"#define RPCC_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION == 105
    binding = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "integration", "rpcc_hip_binding.py")).read()
    assert re.search(r"RPCC_ABI_VERSION = 105\b", binding)


@pytest.mark.parametrize("uniform", (True, False))
def test_container_parser(uniform):
    import rpcc_amd  # noqa: F401
    from rpcc_amd.compress_utils import unpack_bitstream
    from rpcc_amd.pipeline import container_spans
    ns = 4 if uniform else 5
    parts = [bytes([i]) * (3 + 5 * i) for i in range(ns)]
    parts[1] = b""                                               # an empty payload is a payload
    blob = b"".join(struct.pack("i", len(p)) + p for p in parts)
    spans = container_spans(blob, uniform)
    assert [blob[o: o + n] for o, n in spans] == parts == list(unpack_bitstream(blob, uniform).values())
    assert container_spans(blob + b"trailing", uniform) is not None     # unpack_bitstream reads what it needs and ignores the rest
    unpack_bitstream(blob + b"trailing", uniform)
    bad = [blob[:-1], blob[:2], b"", blob[: len(blob) - len(parts[-1]) - 2]]       # payload cut, prefix cut, nothing, last prefix cut
    for k in range(ns):                                          # a negative length, and one past the end, at every position
        off = spans[k][0] - 4
        bad.append(blob[:off] + struct.pack("i", -1) + blob[off + 4:])
        bad.append(blob[:off] + struct.pack("i", len(blob)) + blob[off + 4:])
    for b in bad:
        assert container_spans(b, uniform) is None
        with pytest.raises(ValueError):
            unpack_bitstream(b, uniform)
    if uniform:    # four payloads read with the non-uniform framework's five prefixes: the container ends early
        assert container_spans(blob, False) is None


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from rpcc_amd import _lib
    return _lib.lib()


def test_workspace_bytes(lib):
    for H, W, M in GEOMS + ((16, 1800, 254), (31, 997, 20), (16, 1800, 300), (64, 2048, 100)):
        P = H * W
        sizes = [lib.rpcc_decompress_workspace_bytes(B, P, M) for B in (1, 2, 3, 32, 33, 256)]
        assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])), (H, W, M, sizes)
        assert lib.rpcc_decompress_workspace_bytes(0, P, M) == 0
        assert lib.rpcc_decompress_workspace_bytes(-1, P, M) == 0
        # the decoder's own part is inside: the model part of rpcc_decode's workspace, or the uint16 decoder's whole layout
        inner = lib.rpcc_wide_workspace_bytes(3, P, M, 0) - 4096 if M > 254 else lib.rpcc_codec_workspace_bytes(3, P, M) - 256 - 3 * ((P + 1023) // 1024) * 4
        assert lib.rpcc_decompress_workspace_bytes(3, P, M) >= inner
    assert lib.rpcc_decompress_workspace_bytes(3, 0, 20) == 0 and lib.rpcc_decompress_workspace_bytes(3, 1000, 0) == 0
    assert lib.rpcc_decompress_workspace_bytes(3, 1000, 65534) == 0
