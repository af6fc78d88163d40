"""ctypes binding of librpcc_eval.so (include/rpcc_eval.h), the reconstruction-metrics kernels.  There is no CPU
fallback: if the HIP library is missing, stale or a call fails, this raises."""
import ctypes as C
import os

from ._lib import Binding

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "librpcc_eval.so")

ABI_VERSION = 1        # RPCC_EVAL_ABI_VERSION
BRUTEFORCE = 1         # RPCC_EVAL_BRUTEFORCE
KNN = 12               # RPCC_EVAL_KNN
NSUMS = 10             # RPCC_EVAL_NSUMS
MAX_PIXELS = 1 << 26   # RPCC_EVAL_MAX_PIXELS

_VP, _I, _D, _F = C.c_void_p, C.c_int, C.c_double, C.c_float
_SIGS = {
    "rpcc_eval_version": (C.c_int, []),
    "rpcc_eval_last_error": (C.c_char_p, []),
    "rpcc_eval_workspace_bytes": (C.c_size_t, [_I, _I, _I]),
    "rpcc_eval_nn": (C.c_int, [_VP, _VP, _I, _I, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "rpcc_eval_normals": (C.c_int, [_VP, _I, _I, _I, _D, _I, _VP, _VP, _VP, _VP]),
    "rpcc_eval_metrics": (C.c_int, [_VP, _VP, _I, _I, _I, _VP, _VP, _VP, _F, _VP, _VP, _VP]),
}

_b = Binding("librpcc_eval", LIB_PATH, "rpcc_eval", _SIGS, ABI_VERSION)
lib, check, exported_symbols = _b.lib, _b.check, _b.exported_symbols
