"""The grid cap of the subpixel code pass (rpcc_subpixel_encode in r-pcc_amd/csrc/rpcc_hip.hip, subpixel_code_kernel in subpixel_kernels.h),
read from the sources by regular expression at import, as tests/grid_caps.py reads the intensity launches (whose owner pass the subpixel
entry shares: its caps are grid_caps.INT_*).  tests/subpixel_cases.py sizes `past_the_grid` from the values below, not from literals: a cap
that changes moves the case with it; one that is no longer found raises here."""
import grid_caps as GC

SUB_THREADS = GC._define("subpixel_kernels.h", "SUB_THREADS")                        # pixels of a workgroup and trip of subpixel_code_kernel
SUB_CODE_CAP = GC._product(GC._find("rpcc_hip.hip", r"const unsigned code_wgs = \(unsigned\)std::min<int64_t>\(\(\(int64_t\)B \* P \+ SUB_THREADS - 1\) / SUB_THREADS, (\d+) \* (\d+)\);",
                                    "the grid of subpixel_code_kernel"))
GC._find("rpcc_hip.hip", r"subpixel_code_kernel<<<code_wgs, SUB_THREADS, 0, st>>>", "the launch of subpixel_code_kernel")
GC._find("subpixel_kernels.h", r"for \(int64_t i = \(int64_t\)blockIdx\.x \* SUB_THREADS \+ threadIdx\.x; i < n; i \+= \(int64_t\)gridDim\.x \* SUB_THREADS\)",
         "the pixel loop of subpixel_code_kernel")
INT_FRAME_PIXELS = GC._define("intensity_kernels.h", "INT_FRAME_THREADS") * GC._define("intensity_kernels.h", "INT_PPT")   # pixels of a round of the per-frame kernels


def code_trips(pixels):
    """Trips of workgroup 0 of subpixel_code_kernel over B * P pixels."""
    return GC.trips(pixels, SUB_THREADS, SUB_CODE_CAP)
