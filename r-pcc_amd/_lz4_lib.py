"""ctypes binding of librpcc_lz4.so (include/rpcc_lz4.h), the LZ4 encode / decode / container kernels.  There is no CPU
fallback: if the HIP library is missing, stale or a call fails, this raises."""
import ctypes as C
import os

from ._lib import Binding

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "librpcc_lz4.so")

ABI_VERSION = 1          # RPCC_LZ4_ABI_VERSION
MAX_INPUT = 0x7E000000   # RPCC_LZ4_MAX_INPUT
OK, E_CAPACITY, E_TRUNCATED, E_OFFSET, E_OVERRUN, E_SIZE = 0, -1, -2, -3, -4, -5   # RPCC_LZ4_OK / RPCC_LZ4_E_*

_VP, _I, _I64 = C.c_void_p, C.c_int, C.c_int64
_SIGS = {
    "rpcc_lz4_version": (C.c_int, []),
    "rpcc_lz4_last_error": (C.c_char_p, []),
    "rpcc_lz4_bound": (C.c_size_t, [_I64]),
    "rpcc_lz4_workspace_bytes": (C.c_size_t, [_I64]),
    "rpcc_lz4_encode": (C.c_int, [_VP, _VP, _I64, _VP, _VP, _VP, _VP, _VP]),
    "rpcc_lz4_pack_containers": (C.c_int, [_VP, _VP, _VP, _I64, _I, _VP, _I64, _VP, _VP, _VP, _VP]),
    "rpcc_lz4_decode": (C.c_int, [_VP, _VP, _I64, _VP, _VP, _VP, _VP, _VP, _VP]),
}

_b = Binding("librpcc_lz4", LIB_PATH, "rpcc_lz4", _SIGS, ABI_VERSION)
lib, check, exported_symbols = _b.lib, _b.check, _b.exported_symbols
