"""The threads and the grid cap of the record unpack launch (r-pcc_amd/csrc_records/records_kernels.hip), read from the source by regular
expression at import in the manner of tests/grid_caps.py, and the trip structure of its grid-stride loop.  The `past the grid` case of
tests/test_gpu_records.py is sized from these, not from literals: a cap that changes moves the case with it; one that is no longer found
raises here.  No GPU."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "r-pcc_amd", "csrc_records", "records_kernels.hip")

with open(SRC) as _f:
    _TEXT = _f.read()


def _find(pattern, what):
    m = re.search(pattern, _TEXT, re.M)
    if m is None:
        raise AssertionError("tests/records_caps.py: %s is no longer found in %s (pattern %r): restate the rule" % (what, SRC, pattern))
    return m


REC_THREADS = int(_find(r"^#define[ \t]+REC_THREADS[ \t]+(\d+)", "#define REC_THREADS").group(1))
REC_GRID_CAP = int(_find(r"^#define[ \t]+REC_GRID_CAP[ \t]+(\d+)", "#define REC_GRID_CAP").group(1))
RECORDS_PER_LANE = 2      # one 16-byte load
_find(r"const uint4 v = pairs\[p\];", "the 16-byte load of two records")
_find(r"std::min<int64_t>\(\(npairs \+ REC_THREADS - 1\) / REC_THREADS, REC_GRID_CAP\)", "the capped grid of records_unpack_kernel")
_find(r"for \(int64_t p = \(int64_t\)blockIdx\.x \* REC_THREADS \+ threadIdx\.x; p < npairs; p \+= \(int64_t\)gridDim\.x \* REC_THREADS\)",
      "the grid-stride loop of records_unpack_kernel")

PAIRS_PER_TRIP = REC_THREADS * REC_GRID_CAP       # pairs the whole capped grid takes in one trip


def grid(npairs):
    return max(min(-(-int(npairs) // REC_THREADS), REC_GRID_CAP), 1)


def trips(npairs):
    """Trips of lane 0 of workgroup 0 (the most of any lane) through the loop."""
    return -(-int(npairs) // (grid(npairs) * REC_THREADS))


def past_the_cap_total():
    """A record count whose pairs take the capped grid through a full first trip and a PARTIAL second one that ends inside a workgroup
    and inside a wavefront, and that leaves one record behind the last pair (odd)."""
    return RECORDS_PER_LANE * (PAIRS_PER_TRIP + 5 * REC_THREADS + 37) + 1
