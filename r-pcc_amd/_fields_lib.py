"""ctypes binding of librpcc_fields.so (include/rpcc_fields.h), the .pcd / .ply record unpack kernel.  There is no CPU fallback: if
the HIP library is missing, stale or a call fails, this raises."""
import ctypes as C
import os

from ._lib import Binding

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "librpcc_fields.so")

ABI_VERSION = 1               # RPCC_FIELDS_ABI_VERSION
DESC_WORDS = 16               # RPCC_FIELDS_DESC_WORDS
MAX_STEP = 256                # RPCC_FIELDS_MAX_STEP
MAX_TOTAL = (1 << 31) - 1     # RPCC_FIELDS_MAX_TOTAL
MAX_BATCH = 1 << 20           # RPCC_FIELDS_MAX_BATCH
OK, E_LAYOUT = 0, 1           # RPCC_FIELDS_OK, RPCC_FIELDS_E_LAYOUT

_VP, _I64 = C.c_void_p, C.c_int64
_SIGS = {
    "rpcc_fields_version": (C.c_int, []),
    "rpcc_fields_last_error": (C.c_char_p, []),
    "rpcc_fields_unpack": (C.c_int, [_VP, _I64, _VP, C.c_int, _VP, _I64, _VP, _VP, _VP]),
}

_b = Binding("librpcc_fields", LIB_PATH, "rpcc_fields", _SIGS, ABI_VERSION)
lib, check, exported_symbols = _b.lib, _b.check, _b.exported_symbols
