"""ctypes binding of librpcc_cloud.so (include/rpcc_cloud.h), the .bin row packer for frames with extra points behind their image.  There
is no CPU fallback: if the HIP library is missing, stale or a call fails, this raises."""
import ctypes as C
import os

from ._lib import Binding

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "librpcc_cloud.so")

ABI_VERSION = 1               # RPCC_CLOUD_ABI_VERSION
MAX_BATCH = 65535             # RPCC_CLOUD_MAX_BATCH
MAX_PIXELS = 1 << 26          # RPCC_CLOUD_MAX_PIXELS
ROUND = 4096                  # RPCC_CLOUD_ROUND
OK, E_CAPACITY = 0, 1         # RPCC_CLOUD_OK / RPCC_CLOUD_E_CAPACITY


def table_words(B):
    """RPCC_CLOUD_TABLE_WORDS(B): [0 .. B] offsets, [B + 1] status, then B counts."""
    return 2 * int(B) + 2


_VP, _I, _I64 = C.c_void_p, C.c_int, C.c_int64
_SIGS = {
    "rpcc_cloud_version": (C.c_int, []),
    "rpcc_cloud_last_error": (C.c_char_p, []),
    "rpcc_cloud_pack": (C.c_int, [_VP, _VP, _VP, _I, _I, _VP, _I64, _VP, _VP, _VP, _VP, _I, _VP, _VP]),
}

_b = Binding("librpcc_cloud", LIB_PATH, "rpcc_cloud", _SIGS, ABI_VERSION)
lib, check, exported_symbols = _b.lib, _b.check, _b.exported_symbols
