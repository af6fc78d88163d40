"""ctypes binding of librpcc_seg.so (include/rpcc_seg.h), the DBSCAN segmentation kernels.  There is no CPU fallback: if
the HIP library is missing, stale or a call fails, this raises."""
import ctypes as C
import os

from ._lib import Binding

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "librpcc_seg.so")

ABI_VERSION = 1        # RPCC_SEG_ABI_VERSION
BRUTEFORCE = 1         # RPCC_SEG_BRUTEFORCE
NSTATS = 2             # RPCC_SEG_NSTATS
CAPPED = -1            # RPCC_SEG_CAPPED
MAX_PIXELS = 1 << 26   # RPCC_SEG_MAX_PIXELS

_VP, _I, _D = C.c_void_p, C.c_int, C.c_double
_SIGS = {
    "rpcc_seg_version": (C.c_int, []),
    "rpcc_seg_last_error": (C.c_char_p, []),
    "rpcc_seg_workspace_bytes": (C.c_size_t, [_I, _I, _I]),
    "rpcc_seg_dbscan": (C.c_int, [_VP, _VP, _VP, _I, _I, _I, _D, _I, _I, _VP, _VP, _VP, _VP, _VP]),
}

_b = Binding("librpcc_seg", LIB_PATH, "rpcc_seg", _SIGS, ABI_VERSION)
lib, check, exported_symbols = _b.lib, _b.check, _b.exported_symbols
