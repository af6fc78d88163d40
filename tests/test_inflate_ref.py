"""tests/inflate_ref.py, the Python statement of the device inflate, against gzip.decompress: the same bytes on every valid stream, OK
exactly where gzip.decompress returns on every bit flip and truncation, and the stated status on every hand-built stream.  No GPU needed."""
import gzip

import pytest

import inflate_cases as C
import inflate_ref as R


@pytest.mark.parametrize("name", sorted(C.valid()))
def test_valid_streams(name):
    stream, plain, check = C.valid()[name]
    assert gzip.decompress(stream) == plain
    st, got, rep = R.inflate(stream, cap=len(plain), report=True)
    assert st == R.OK and got == plain
    check(rep)


def test_empty_stream_is_empty_output():
    assert gzip.decompress(b"") == b"" and R.inflate(b"") == (R.OK, b"")


def test_small_members_cover_the_block_types():
    kinds = [set(R.inflate(m, report=True)[2]["blocks"]) for m, _ in C.small_members()]
    assert kinds == [{C.DYNAMIC}, {C.FIXED}, {C.STORED}, {C.DYNAMIC}]
    assert all(150 <= len(m) <= 400 for m, _ in C.small_members())


@pytest.mark.parametrize("which", ["flips", "truncations"])
def test_ok_exactly_where_gzip_decompress_returns(which):
    streams = getattr(C, which)()
    accepted = 0
    for k, (stream, cap) in enumerate(streams):
        ok, plain = C.gzip_accepts(stream)
        st, got = R.inflate(stream, cap=cap)
        assert (st == R.OK) == ok, (which, k, R.NAMES[st])
        if ok:
            assert got == plain, (which, k)
            accepted += 1
    if which == "flips":
        assert 0 < accepted < len(streams) // 8     # the header's ignored fields, and nothing else
    else:
        assert accepted == 0


@pytest.mark.parametrize("name", sorted(C.hand_built()))
def test_hand_built_streams(name):
    stream, cap, want = C.hand_built()[name]
    st, got = R.inflate(stream, cap=cap)
    assert st == want, (R.NAMES[st], R.NAMES[want])
    ok, plain = C.gzip_accepts(stream)
    if name == "two_members":
        assert ok and plain == got * 2      # gzip.decompress concatenates members; the decoder refuses the second
    elif name in ("one_byte_over",):
        assert ok and len(plain) == cap + 1
    else:
        assert ok == (st == R.OK)
        if ok:
            assert got == plain and len(got) == cap
