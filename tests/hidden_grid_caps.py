"""The grid cap of the hidden_points row passes (rpcc_hidden_encode in r-pcc_amd/csrc/rpcc_hip.hip: hidden_count_kernel, hidden_scatter_kernel
and hidden_rank_kernel of hidden_kernels.h share one grid), read from the sources by regular expression at import, as tests/grid_caps.py
reads the intensity launches (whose owner pass the entry shares: its caps are grid_caps.INT_*).  tests/hidden_cases.py sizes
`past_the_grid` from the values below, not from literals: a cap that changes moves the case with it; one that is no longer found raises here."""
import grid_caps as GC

HID_THREADS = GC._define("hidden_kernels.h", "HID_THREADS")                          # rows of a workgroup and trip of the three row passes
HID_ROW_CAP = GC._product(GC._find("rpcc_hip.hip", r"const unsigned row_wgs = \(unsigned\)std::min<int64_t>\(\(total \+ HID_THREADS - 1\) / HID_THREADS, (\d+) \* (\d+)\);",
                                   "the grid of the hidden_points row passes"))
for _kernel, _var in (("hidden_count_kernel", "i"), ("hidden_scatter_kernel", "i"), ("hidden_rank_kernel", "j")):
    GC._find("rpcc_hip.hip", r"%s<<<row_wgs, HID_THREADS, 0, st>>>" % _kernel, "the launch of " + _kernel)
    GC._find("hidden_kernels.h", r"for \(int64_t %s = \(int64_t\)blockIdx\.x \* HID_THREADS \+ threadIdx\.x; %s < total; %s \+= \(int64_t\)gridDim\.x \* HID_THREADS\)"
             % (_var, _var, _var), "the row loop of " + _kernel)
INT_FRAME_PIXELS = GC._define("intensity_kernels.h", "INT_FRAME_THREADS") * GC._define("intensity_kernels.h", "INT_PPT")   # pixels of a round of the per-frame kernels
HID_CAP = GC._define("hidden_kernels.h", "HID_CAP")


def row_trips(total):
    """Trips of workgroup 0 of the row passes over `total` rows."""
    return GC.trips(total, HID_THREADS, HID_ROW_CAP)
