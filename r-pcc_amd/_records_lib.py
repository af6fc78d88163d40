"""ctypes binding of librpcc_records.so (include/rpcc_records.h), the NCLT record unpack kernel.  There is no CPU fallback: if
the HIP library is missing, stale or a call fails, this raises."""
import ctypes as C
import os

from ._lib import Binding

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "librpcc_records.so")

ABI_VERSION = 1               # RPCC_RECORDS_ABI_VERSION
RECORD_BYTES = 8              # RPCC_RECORDS_BYTES
MAX_TOTAL = (1 << 31) - 1     # RPCC_RECORDS_MAX_TOTAL

_VP, _I64 = C.c_void_p, C.c_int64
_SIGS = {
    "rpcc_records_version": (C.c_int, []),
    "rpcc_records_last_error": (C.c_char_p, []),
    "rpcc_records_unpack": (C.c_int, [_VP, _I64, _VP, _VP]),
}

_b = Binding("librpcc_records", LIB_PATH, "rpcc_records", _SIGS, ABI_VERSION)
lib, check, exported_symbols = _b.lib, _b.check, _b.exported_symbols
