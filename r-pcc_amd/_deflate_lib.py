"""ctypes binding of librpcc_deflate.so (include/rpcc_deflate.h), the gzip / deflate encoder kernels.  There is no CPU
fallback: if the HIP library is missing, stale or a call fails, this raises."""
import ctypes as C
import os

from ._lib import Binding

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "librpcc_deflate.so")

ABI_VERSION = 1          # RPCC_DEFLATE_ABI_VERSION
MAX_INPUT = 0x7E000000   # RPCC_DEFLATE_MAX_INPUT
E_CAPACITY = -1          # RPCC_DEFLATE_E_CAPACITY

_VP, _I64 = C.c_void_p, C.c_int64
_SIGS = {
    "rpcc_deflate_version": (C.c_int, []),
    "rpcc_deflate_last_error": (C.c_char_p, []),
    "rpcc_deflate_bound": (C.c_size_t, [_I64]),
    "rpcc_deflate_workspace_bytes": (C.c_size_t, [_I64, _I64]),
    "rpcc_deflate_encode": (C.c_int, [_VP, _VP, _I64, _I64, _VP, _VP, _VP, _VP, _VP, _VP]),
}

_b = Binding("librpcc_deflate", LIB_PATH, "rpcc_deflate", _SIGS, ABI_VERSION)
lib, check, exported_symbols = _b.lib, _b.check, _b.exported_symbols
