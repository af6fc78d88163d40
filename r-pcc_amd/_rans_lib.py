"""ctypes binding of librpcc_rans.so (include/rpcc_rans.h), the chunk-parallel rANS encode / decode kernels.  There is no CPU
fallback: if the HIP library is missing, stale or a call fails, this raises."""
import ctypes as C
import os

from ._lib import Binding

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "librpcc_rans.so")

ABI_VERSION = 1              # RPCC_RANS_ABI_VERSION
MAX_INPUT = 0x7E000000       # RPCC_RANS_MAX_INPUT
DEFAULT_CHUNK_LOG2 = 15      # RPCC_RANS_DEFAULT_CHUNK_LOG2
OK, E_CAPACITY, E_HEADER, E_TRUNCATED, E_TABLE, E_DIRECTORY, E_STATE, E_PAYLOAD = 0, -1, -2, -3, -4, -5, -6, -7   # RPCC_RANS_OK / RPCC_RANS_E_*
FILTER_NONE, FILTER_DELTA = 0, 1   # RPCC_RANS_FILTER_*


def width_word(width, filter=FILTER_NONE):
    """RPCC_RANS_WIDTH_WORD: the per-stream width word of rpcc_rans_encode -- the element size in bits 0-7, the filter in bits 8-15."""
    return int(width) | int(filter) << 8


_VP, _I, _I64 = C.c_void_p, C.c_int, C.c_int64
_SIGS = {
    "rpcc_rans_version": (C.c_int, []),
    "rpcc_rans_last_error": (C.c_char_p, []),
    "rpcc_rans_bound": (C.c_size_t, [_I64]),
    "rpcc_rans_workspace_bytes": (C.c_size_t, [_I64, _I64, _I]),
    "rpcc_rans_encode": (C.c_int, [_VP, _VP, _VP, _I64, _I64, _I, _VP, _VP, _VP, _VP, _VP, _VP]),
    "rpcc_rans_decode": (C.c_int, [_VP, _VP, _I64, _VP, _VP, _VP, _VP, _VP, _VP]),
}

_b = Binding("librpcc_rans", LIB_PATH, "rpcc_rans", _SIGS, ABI_VERSION)
lib, check, exported_symbols = _b.lib, _b.check, _b.exported_symbols
