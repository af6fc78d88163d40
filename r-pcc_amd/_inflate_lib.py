"""ctypes binding of librpcc_inflate.so (include/rpcc_inflate.h), the gzip / deflate decoder kernel.  There is no CPU
fallback: if the HIP library is missing, stale or a call fails, this raises."""
import ctypes as C
import os

from ._lib import Binding

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "librpcc_inflate.so")

ABI_VERSION = 1          # RPCC_INFLATE_ABI_VERSION
OK = 0                   # RPCC_INFLATE_OK, RPCC_INFLATE_E_*
E_TRUNCATED, E_HEADER, E_BTYPE, E_STORED, E_TABLE, E_SYMBOL, E_OFFSET, E_OVERRUN, E_CRC, E_SIZE, E_TRAILING = range(-2, -13, -1)

_VP, _I64 = C.c_void_p, C.c_int64
_SIGS = {
    "rpcc_inflate_version": (C.c_int, []),
    "rpcc_inflate_last_error": (C.c_char_p, []),
    "rpcc_inflate_decode": (C.c_int, [_VP, _VP, _I64, _VP, _VP, _VP, _VP, _VP, _VP]),
}

_b = Binding("librpcc_inflate", LIB_PATH, "rpcc_inflate", _SIGS, ABI_VERSION)
lib, check, exported_symbols = _b.lib, _b.check, _b.exported_symbols
