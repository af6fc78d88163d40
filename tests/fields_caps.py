"""The threads, the tile rule and the grid cap of the field unpack launch (r-pcc_amd/csrc_fields/fields_kernels.hip and fields_rule.h), read
from the source by regular expression at import in the manner of tests/records_caps.py.  The point counts of tests/test_gpu_fields.py are
sized from these, not from literals: a rule that changes moves the cases with it; one that is no longer found raises here.  No GPU."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "r-pcc_amd", "csrc_fields", "fields_kernels.hip")
RULE = os.path.join(ROOT, "r-pcc_amd", "csrc_fields", "fields_rule.h")

with open(SRC) as _f:
    _TEXT = _f.read()
with open(RULE) as _f:
    _RULE = _f.read()


def _find(pattern, what, text=None, src=SRC):
    m = re.search(pattern, _TEXT if text is None else text, re.M)
    if m is None:
        raise AssertionError("tests/fields_caps.py: %s is no longer found in %s (pattern %r): restate the rule" % (what, src, pattern))
    return m


FLD_THREADS = int(_find(r"^#define[ \t]+FLD_THREADS[ \t]+(\d+)", "#define FLD_THREADS").group(1))
FLD_GRID_CAP = int(_find(r"^#define[ \t]+FLD_GRID_CAP[ \t]+(\d+)", "#define FLD_GRID_CAP").group(1))
STAGE_BYTES = int(_find(r"^#define[ \t]+FIELDS_STAGE_BYTES[ \t]+(\d+)", "#define FIELDS_STAGE_BYTES", _RULE, RULE).group(1))
TILE_MAX_ROWS = int(_find(r"^#define[ \t]+FIELDS_TILE_MAX_ROWS[ \t]+(\d+)", "#define FIELDS_TILE_MAX_ROWS", _RULE, RULE).group(1))
MAX_STEP = int(_find(r"^#define[ \t]+FIELDS_MAX_STEP[ \t]+(\d+)", "#define FIELDS_MAX_STEP", _RULE, RULE).group(1))
_find(r"const int64_t r = FIELDS_STAGE_BYTES / max_step;\s*return \(int\)\(r < FIELDS_TILE_MAX_ROWS \? r : FIELDS_TILE_MAX_ROWS\);", "the tile rule", _RULE, RULE)
_find(r"static_assert\(FIELDS_TILE_MAX_ROWS % FLD_THREADS == 0", "a full tile's points divide among the lanes")
_find(r"for \(int r = lane; r < cnt; r \+= FLD_THREADS\)", "the lanes' loop over a tile's points")
_find(r"v = \*\(const uint4 \*\)\(bytes \+ o\);", "the aligned 16-byte load of the stage")
_find(r"for \(int64_t t = blockIdx\.x; t < ntiles; t \+= gridDim\.x\)", "the tile loop of fields_unpack_kernel")
_find(r"for \(int b = blockIdx\.y; b < B; b \+= gridDim\.y\)", "the frame loop of fields_unpack_kernel")
_find(r"const int64_t fy = std::min<int64_t>\(B, FLD_GRID_CAP\);", "the capped grid: frames")
_find(r"const int64_t per_frame = \(total / B \+ FIELDS_TILE_MAX_ROWS - 1\) / FIELDS_TILE_MAX_ROWS;", "the capped grid: tiles of an average frame")
_find(r"const int64_t fx = std::max<int64_t>\(std::min<int64_t>\(per_frame, FLD_GRID_CAP / fy\), 1\);", "the capped grid: tiles")


def tile_rows(max_step):
    return min(STAGE_BYTES // int(max_step), TILE_MAX_ROWS)


def grid(total, B):
    """(fx, fy) of the launch for B frames of `total` rows together."""
    fy = min(B, FLD_GRID_CAP)
    per_frame = -(-(total // B) // TILE_MAX_ROWS)
    return max(min(per_frame, FLD_GRID_CAP // fy), 1), fy


def point_counts(max_step):
    """0, 1, a tile less one, a tile, a tile and one, and several tiles plus a remainder that ends inside a wavefront."""
    t = tile_rows(max_step)
    return (0, 1, t - 1, t, t + 1, 3 * t + 37)
