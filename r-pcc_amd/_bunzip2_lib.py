"""ctypes binding of librpcc_bunzip2.so (include/rpcc_bunzip2.h), the bzip2 decoder kernel.  There is no CPU
fallback: if the HIP library is missing, stale or a call fails, this raises."""
import ctypes as C
import os

from ._lib import Binding

_HERE = os.path.dirname(os.path.abspath(__file__))
# RPCC_BUNZIP2_LIB: developer knob -- another build of the same ABI (tools_dev/bunzip2_time.py --lib)
LIB_PATH = os.environ.get("RPCC_BUNZIP2_LIB") or os.path.join(_HERE, "lib", "librpcc_bunzip2.so")

ABI_VERSION = 1          # RPCC_BUNZIP2_ABI_VERSION
MAX_BLOCK = 900000       # RPCC_BUNZIP2_MAX_BLOCK
OK = 0                   # RPCC_BUNZIP2_OK, RPCC_BUNZIP2_E_*
(E_TRUNCATED, E_HEADER, E_MAGIC, E_RANDOMISED, E_TABLE, E_SYMBOL, E_ORIGPTR, E_OVERRUN, E_CRC, E_WORK, E_TRAILING,
 E_RLE) = range(-2, -14, -1)

_VP, _I64 = C.c_void_p, C.c_int64
_SIGS = {
    "rpcc_bunzip2_version": (C.c_int, []),
    "rpcc_bunzip2_last_error": (C.c_char_p, []),
    "rpcc_bunzip2_stream_work_bytes": (_I64, [_I64]),
    "rpcc_bunzip2_decode": (C.c_int, [_VP, _VP, _I64, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
}

_b = Binding("librpcc_bunzip2", LIB_PATH, "rpcc_bunzip2", _SIGS, ABI_VERSION)
lib, check, exported_symbols = _b.lib, _b.check, _b.exported_symbols
