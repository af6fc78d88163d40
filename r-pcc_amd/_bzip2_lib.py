"""ctypes binding of librpcc_bzip2.so (include/rpcc_bzip2.h), the bzip2 encoder kernels.  There is no CPU fallback: if the HIP
library is missing, stale or a call fails, this raises."""
import ctypes as C
import os

from ._lib import Binding

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "librpcc_bzip2.so")

ABI_VERSION = 1          # RPCC_BZIP2_ABI_VERSION
MAX_INPUT = 0x7E000000   # RPCC_BZIP2_MAX_INPUT
E_CAPACITY = -1          # RPCC_BZIP2_E_CAPACITY

_VP, _I64, _I = C.c_void_p, C.c_int64, C.c_int
_SIGS = {
    "rpcc_bzip2_version": (C.c_int, []),
    "rpcc_bzip2_last_error": (C.c_char_p, []),
    "rpcc_bzip2_bound": (C.c_size_t, [_I64, _I]),
    "rpcc_bzip2_workspace_bytes": (C.c_size_t, [_I64, _I64, _I]),
    "rpcc_bzip2_encode": (C.c_int, [_VP, _VP, _I64, _I64, _I, _VP, _VP, _VP, _VP, _VP, _VP]),
}

_b = Binding("librpcc_bzip2", LIB_PATH, "rpcc_bzip2", _SIGS, ABI_VERSION)
lib, check, exported_symbols = _b.lib, _b.check, _b.exported_symbols
