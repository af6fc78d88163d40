"""ctypes binding of librpcc_filter.so (include/rpcc_filter.h), the radius outlier removal kernels.  There is no CPU fallback: if
the HIP library is missing, stale or a call fails, this raises."""
import ctypes as C
import os

from ._lib import Binding

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "librpcc_filter.so")

ABI_VERSION = 1        # RPCC_FILTER_ABI_VERSION
BRUTEFORCE = 1         # RPCC_FILTER_BRUTEFORCE
NSTATS = 2             # RPCC_FILTER_NSTATS
TILE = 256             # RPCC_FILTER_TILE
TILE_LIST = 256        # RPCC_FILTER_TILE_LIST
MAX_POINTS = 1 << 30   # RPCC_FILTER_MAX_POINTS

_VP, _I, _I64, _D = C.c_void_p, C.c_int, C.c_int64, C.c_double
_SIGS = {
    "rpcc_filter_version": (C.c_int, []),
    "rpcc_filter_last_error": (C.c_char_p, []),
    "rpcc_filter_workspace_bytes": (C.c_size_t, [_I64, _I]),
    "rpcc_filter_radius": (C.c_int, [_VP, _I, _VP, _I64, _I, _D, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
}

_b = Binding("librpcc_filter", LIB_PATH, "rpcc_filter", _SIGS, ABI_VERSION)
lib, check, exported_symbols = _b.lib, _b.check, _b.exported_symbols
