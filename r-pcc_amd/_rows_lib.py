"""ctypes binding of librpcc_rows.so (include/rpcc_rows.h), the .bin row packer.  There is no CPU fallback: if the HIP library is
missing, stale or a call fails, this raises."""
import ctypes as C
import os

from ._lib import Binding

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "librpcc_rows.so")

ABI_VERSION = 1               # RPCC_ROWS_ABI_VERSION
MAX_BATCH = 65535             # RPCC_ROWS_MAX_BATCH
MAX_PIXELS = 1 << 26          # RPCC_ROWS_MAX_PIXELS
ROUND = 4096                  # RPCC_ROWS_ROUND
OK, E_CAPACITY = 0, 1         # RPCC_ROWS_OK / RPCC_ROWS_E_CAPACITY


def table_words(B):
    """RPCC_ROWS_TABLE_WORDS(B): [0 .. B] offsets, [B + 1] status, then B counts."""
    return 2 * int(B) + 2


_VP, _I, _I64 = C.c_void_p, C.c_int, C.c_int64
_SIGS = {
    "rpcc_rows_version": (C.c_int, []),
    "rpcc_rows_last_error": (C.c_char_p, []),
    "rpcc_rows_pack": (C.c_int, [_VP, _VP, _VP, _I, _I, _VP, _I64, _VP, _VP, _VP, _VP]),
}

_b = Binding("librpcc_rows", LIB_PATH, "rpcc_rows", _SIGS, ABI_VERSION)
lib, check, exported_symbols = _b.lib, _b.check, _b.exported_symbols
