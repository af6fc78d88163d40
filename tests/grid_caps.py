"""The grid caps of the intensity and the beam-table launches (r-pcc_amd/csrc/rpcc_hip.hip, intensity_kernels.h, beams_kernels.h), read
from the sources by regular expression at import, and the trip structure of their grid-stride loops restated in numpy (no GPU;
tests/test_intensity_ref.py and tests/test_beam_table_ref.py assert with it that the `past the grid` cases take every loop through a second
trip and the LDS queues through a drain that leaves a remainder; tests/intensity_cases.py and tests/beam_table_cases.py size those cases
from the values below, not from literals).  A cap that changes moves the cases with it; one that is no longer found raises here."""
import functools
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "r-pcc_amd", "csrc")


@functools.lru_cache(maxsize=None)
def _text(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _find(name, pattern, what):
    m = re.search(pattern, _text(name), re.M)
    if m is None:
        raise AssertionError("tests/grid_caps.py: %s is no longer found in r-pcc_amd/csrc/%s (pattern %r): restate the rule" % (what, name, pattern))
    return m


def _define(name, macro):
    return int(_find(name, r"^#define[ \t]+%s[ \t]+\(?(\d+)\)?" % macro, "#define " + macro).group(1))


def _product(m):
    return int(np.prod([int(v) for v in m.groups()]))


# ---- intensity (rpcc_intensity_encode, rpcc_hip.hip) -----------------------------------------------------------------------------------
INT_THREADS = _define("intensity_kernels.h", "INT_THREADS")                         # rows of a chunk of intensity_owner_kernel
INT_FILL_THREADS = int(_find("rpcc_hip.hip", r"intensity_fill_kernel<<<fill_wgs, (\d+), 0, st>>>\(l\.owner, l\.lastz, l\.flags, px, B, false, P\)",
                             "the workgroup size of intensity_fill_kernel").group(1))
INT_FILL_CAP = int(_find("rpcc_hip.hip", r"const unsigned fill_wgs = \(unsigned\)std::min<int64_t>\(\(px \+ 255\) / 256, (\d+)\);",
                         "the grid of intensity_fill_kernel").group(1))
INT_OWNER_CAP = _product(_find("rpcc_hip.hip", r"const unsigned wgs = \(unsigned\)std::min<int64_t>\(\(total \+ INT_THREADS - 1\) / INT_THREADS, (\d+) \* (\d+)\);",
                               "the grid of intensity_owner_kernel<false>"))
INT_FIXUP_CAP = int(_find("rpcc_hip.hip", r"intensity_owner_kernel<true><<<std::min\(wgs, (\d+)u\), INT_THREADS, 0, st>>>",
                          "the grid of intensity_owner_kernel<true>").group(1))
_find("intensity_kernels.h", r"for \(int64_t c = \(int64_t\)blockIdx\.x \* INT_THREADS; c < total; c \+= \(int64_t\)gridDim\.x \* INT_THREADS\)",
      "the chunk loop of intensity_owner_kernel")
_find("intensity_kernels.h", r"if \(n >= INT_THREADS\) \{", "the drain of intensity_owner_kernel's queue")

# ---- beam table (launch_project_beams, beams_kernels.h) ----------------------------------------------------------------------------------
BEAMS_THREADS = _define("beams_kernels.h", "BEAMS_THREADS")
BEAMS_PPT = _define("beams_kernels.h", "BEAMS_PPT")
BEAMS_CHUNK = BEAMS_PPT * BEAMS_THREADS                                              # points of a chunk of beams_pix_kernel
_m = _find("beams_kernels.h", r"beams_fill_kernel<<<\(unsigned\)std::min<int64_t>\(\(n \+ 255\) / 256, (\d+)\), (\d+), 0, st>>>", "the grid of beams_fill_kernel")
BEAMS_FILL_CAP, BEAMS_FILL_THREADS = int(_m.group(1)), int(_m.group(2))
BEAMS_PIX_CAP = _product(_find("beams_kernels.h", r"const unsigned wgs = \(unsigned\)std::min<int64_t>\(nck, (\d+) \* (\d+)\);", "the grid of beams_pix_kernel"))
_m = _find("beams_kernels.h", r"beams_write_kernel<<<\(unsigned\)std::min<int64_t>\(\(total \+ 255\) / 256, (\d+)\), (\d+), 0, st>>>", "the grid of beams_write_kernel")
BEAMS_WRITE_CAP, BEAMS_WRITE_THREADS = int(_m.group(1)), int(_m.group(2))
_find("beams_kernels.h", r"const int64_t CH = \(int64_t\)BEAMS_PPT \* BEAMS_THREADS, nck = \(total \+ CH - 1\) / CH;\s*\n\s*for \(int64_t k = blockIdx\.x; k < nck; k \+= gridDim\.x\)",
      "the chunk loop of beams_pix_kernel")
_find("beams_kernels.h", r"while \(n >= BEAMS_THREADS\) \{", "the drain of beams_pix_kernel's queue")


# ---- the loops -------------------------------------------------------------------------------------------------------------------------
def grid(n, per_wg, cap):
    """Workgroups of a launch over n elements, per_wg per workgroup and trip."""
    return int(min(-(-int(n) // per_wg), cap))


def trips(n, per_wg, cap):
    """Trips of workgroup 0 (the most of any workgroup) through a grid-stride loop over n elements; 0 for an empty launch."""
    return -(-(-(-int(n) // per_wg)) // grid(n, per_wg, cap)) if n > 0 else 0


def fill_trips(pixels, threads, cap):
    """intensity_fill_kernel / beams_fill_kernel over B * P pixels."""
    return trips(pixels, threads, cap)


def owner_rows(total, w, r, cap=INT_OWNER_CAP):
    """intensity_owner_kernel: the rows [first, end) of the launch that workgroup w takes in trip r (end <= first: none).  cap: INT_OWNER_CAP
    for the first pass, INT_FIXUP_CAP for the fix-up pass (its grid is the smaller of the two)."""
    first = (w + r * grid(total, INT_THREADS, min(cap, INT_OWNER_CAP))) * INT_THREADS
    return first, min(first + INT_THREADS, int(total))


def pix_rows(total, w, r):
    """beams_pix_kernel: the points [first, end) that workgroup w takes in trip r."""
    first = (w + r * grid(total, BEAMS_CHUNK, BEAMS_PIX_CAP)) * BEAMS_CHUNK
    return first, min(first + BEAMS_CHUNK, int(total))


def chunk_counts(mask, total, per_chunk):
    """Rows of every chunk for which mask holds: i64 [ceil(total / per_chunk)]."""
    nck = -(-int(total) // per_chunk)
    m = np.zeros(nck * per_chunk, np.int64)
    m[:total] = np.asarray(mask[:total], dtype=np.int64)
    return m.reshape(nck, per_chunk).sum(1)


def single_turn_losses(queued, total, per_chunk, cap, drain):
    """A model of the mistake `one turn of the drain per chunk` (an `if` where beams_pix_kernel has its `while`): the queue takes a chunk's
    queued rows in row order behind what it carried, one drain takes the top `drain` entries, and what then still stands above
    drain - 1 entries is lost.  -> bool [total], the rows lost.  (The order inside a chunk is the wavefronts' on the device; how MANY rows
    a chunk loses does not depend on it.)"""
    lost = np.zeros(total, bool)
    G = grid(total, per_chunk, cap)
    nck = -(-int(total) // per_chunk)
    for w in range(G):
        queue = np.zeros(0, np.int64)
        for k in range(w, nck, G):
            queue = np.concatenate([queue, k * per_chunk + np.flatnonzero(queued[k * per_chunk: (k + 1) * per_chunk])])
            if queue.shape[0] >= drain:
                queue = queue[:-drain]
            if queue.shape[0] >= drain:
                lost[queue[drain - 1:]] = True
                queue = queue[: drain - 1]
    return lost


def queue_facts(queued, maybe, total, per_chunk, cap, drain):
    """What the LDS queue of the persistent workgroups certainly goes through.  queued: bool [total], rows that take the exact path by rule
    (a lower bound of what a chunk adds to the queue); maybe: bool [total], rows that are not certain to take the fast path (an upper
    bound); drain: the queue is emptied `drain` entries at a time once it holds that many.  -> dict of workgroup / chunk indices:
      full        chunks that add at least a whole drain by themselves (`full_n`: how many drains the fullest is good for)
      remainder   workgroups whose first chunk adds 1 .. drain - 1 (so no drain in trip 1, and at least one row of it goes the fast way),
                  and whose first two chunks together add more than a drain: the drain of trip 2 takes the top and leaves a remainder
      carried     workgroups whose first two chunks each add less than a drain and together at least one: only the carried queue drains
      refilled    workgroups whose first chunk is exactly one drain of queued rows and whose second chunk queues at least one
      tail        workgroups of two trips or more with a non-empty queue behind the loop (no multiple of `drain` between the bounds)"""
    lo, up = chunk_counts(queued, total, per_chunk), chunk_counts(maybe, total, per_chunk)
    assert np.all(lo <= up)
    G = grid(total, per_chunk, cap)
    two = np.arange(min(max(lo.shape[0] - G, 0), G))             # workgroups with a second trip
    a_lo, a_up, b_lo, b_up = lo[two], up[two], lo[two + G], up[two + G]
    sum_lo, sum_up = np.zeros(G, np.int64), np.zeros(G, np.int64)
    for r in range(trips(total, per_chunk, cap)):
        part = lo[r * G: (r + 1) * G]
        sum_lo[: part.shape[0]] += part
        sum_up[: part.shape[0]] += up[r * G: (r + 1) * G]
    tail = two[(sum_lo[two] >= 1) & (sum_lo[two] // drain == sum_up[two] // drain) & (sum_lo[two] % drain >= 1)]
    return dict(grid=G, trips=trips(total, per_chunk, cap), full=np.flatnonzero(lo >= drain), full_n=int(lo.max() // drain) if lo.size else 0,
                remainder=two[(a_lo >= 1) & (a_up <= drain - 1) & (a_up < per_chunk) & (a_lo + b_lo > drain)],
                carried=two[(a_up < drain) & (b_up < drain) & (a_lo + b_lo >= drain)],
                refilled=two[(a_lo == drain) & (a_up == drain) & (b_lo >= 1)], tail=tail)
