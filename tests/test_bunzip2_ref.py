"""tests/bunzip2_ref.py, the Python statement of the device bunzip2, against bz2.decompress: the same bytes on every valid stream; on every
bit flip, truncation and hand-built stream OK exactly where bz2.decompress returns, E_OVERRUN only where it returns that many bytes, and
every other status but the three that are not comparable only where it raises.  No GPU needed."""
import collections

import pytest

import bunzip2_cases as C
import bunzip2_ref as R

NOT_COMPARABLE = (R.E_WORK, R.E_TRAILING, R.E_RANDOMISED)     # a slot too small; what libbz2 reads and the kernel leaves to the host


def _held_to_bz2(name, stream, cap, slot):
    """What the reference owes bz2.decompress on one stream -> the reference's status."""
    st, got, size, used = R.bunzip2(stream, cap=cap, nblock_max=slot)
    ok, plain = C.bz2_accepts(stream)
    if st == R.OK:
        assert ok and got == plain and size == len(plain) and used == len(stream), name
    elif st == R.E_OVERRUN:
        assert ok and size == len(plain) > cap and got == plain[:cap], name
    elif st not in NOT_COMPARABLE:
        assert not ok, (name, R.NAMES[st])
    assert 0 <= used <= len(stream), name
    return st


@pytest.mark.parametrize("name", sorted(C.valid()))
def test_valid_streams(name):
    stream, plain = C.valid()[name]
    st, got, size, used, rep = R.bunzip2(stream, cap=len(plain), nblock_max=R.block_bound(int(stream[3:4]), len(plain)), report=True)
    assert st == R.OK and got == plain and size == len(plain) and used == len(stream)
    if name == "random_level1":
        assert rep["blocks"] == 3
    if name == "abc_period":
        assert rep["cycle_short"]
    if name == "len0":
        assert rep["blocks"] == 0
    if name.startswith("golden_"):
        assert rep["blocks"] == 1 and stream[:4] == b"BZh9"


def test_golden_members_are_the_example_frames():
    sizes = [(len(m), len(C.valid()["golden_" + k][1])) for k, m in C.golden_members().items()]
    assert sizes == [(4762, 16000), (1841, 12134), (590, 1632), (29126, 188106)]


def test_the_block_bound_holds_on_every_valid_stream():
    for name, (stream, plain) in C.valid().items():
        slot = R.block_bound(int(stream[3:4]), len(plain))
        assert R.bunzip2(stream, cap=len(plain), nblock_max=slot)[0] == R.OK, name
    worst = C.rle1(b"abcde" * 2 + b"q" * 4)          # four equal bytes and a count of zero: five bytes for four
    assert len(worst) == 15 and R.block_bound(9, 14) >= len(worst)


def test_flips():
    streams = C.flips()
    assert 130 * 8 <= len(streams) <= 180 * 8
    count = collections.Counter(_held_to_bz2("flip%d" % k, s, C.FLIP_CAP, C.FLIP_BLOCK) for k, s in enumerate(streams))
    # counted on the CPU when this test was written; E_WORK, which cannot be compared, takes none of them
    assert {R.NAMES[k]: v for k, v in count.items()} == {"E_HEADER": 30, "OK": 5, "E_MAGIC": 96, "E_CRC": 637, "E_RANDOMISED": 1, "E_ORIGPTR": 46,
                                                         "E_TABLE": 45, "E_SYMBOL": 208, "E_RLE": 4}
    assert count[R.E_WORK] == 0 <= len(streams) // 100


def test_truncations():
    streams = C.truncations()
    count = collections.Counter(_held_to_bz2("cut%d" % k, s, C.FLIP_CAP, C.FLIP_BLOCK) for k, s in enumerate(streams))
    assert count == {R.E_TRUNCATED: len(streams)}


@pytest.mark.parametrize("name", sorted(C.hand_built()))
def test_hand_built_streams(name):
    stream, cap, slot, want = C.hand_built()[name]
    st = _held_to_bz2(name, stream, cap, slot)
    if want is not None:
        assert st == want, (R.NAMES[st], R.NAMES[want])
    ok, plain = C.bz2_accepts(stream)
    if name in ("second_stream", "trailing_zeros", "randomised"):
        assert ok                                    # libbz2 reads these; bunzip2_codec hands them to it
    if name == "trailing_partial_stream":
        assert not ok                                # ... and it refuses this one
    if name in ("oversubscribed", "incomplete", "code_20_bits", "tables_6", "selectors_18010", "count_byte_is_run_byte"):
        assert ok and st == R.OK


def test_hand_built_tables_are_what_they_say():
    rep = {k: R.bunzip2(C.hand_built()[k][0], report=True)[4] for k in ("tables_2", "tables_6", "code_20_bits", "three_blocks")}
    assert rep["tables_2"]["groups"] == [2] and rep["tables_6"]["groups"] == [6]
    assert rep["code_20_bits"]["max_code_length"] == 20 and rep["three_blocks"]["blocks"] == 3


def test_rle_state_resets_at_every_block():
    """Three equal bytes end one block and the same byte opens the next: no count byte follows."""
    s = C.stream([(b"ab" + b"c" * 3, {}), (b"c" + b"\x05" + b"de", {})])
    st, got, _, _ = R.bunzip2(s)
    ok, plain = C.bz2_accepts(s)
    assert st == R.OK and ok and got == plain == b"abccc" + b"c\x05de"


def test_empty_input_is_truncated():
    assert R.bunzip2(b"")[0] == R.E_TRUNCATED
