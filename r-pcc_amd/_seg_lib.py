"""ctypes binding of librpcc_seg.so (include/rpcc_seg.h), the DBSCAN segmentation kernels.  There is no CPU fallback: if
the HIP library is missing, stale or a call fails, this raises."""
import ctypes as C
import os

import torch  # noqa: F401  (imported first so the library binds to the HIP runtime torch already loaded)

from ._lib import RpccError

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "librpcc_seg.so")

ABI_VERSION = 1        # RPCC_SEG_ABI_VERSION
BRUTEFORCE = 1         # RPCC_SEG_BRUTEFORCE
NSTATS = 2             # RPCC_SEG_NSTATS
CAPPED = -1            # RPCC_SEG_CAPPED
MAX_PIXELS = 1 << 26   # RPCC_SEG_MAX_PIXELS

_VP, _I, _D = C.c_void_p, C.c_int, C.c_double
_SIGS = {
    "rpcc_seg_version": (C.c_int, []),
    "rpcc_seg_last_error": (C.c_char_p, []),
    "rpcc_seg_workspace_bytes": (C.c_size_t, [_I, _I, _I]),
    "rpcc_seg_dbscan": (C.c_int, [_VP, _VP, _VP, _I, _I, _I, _D, _I, _I, _VP, _VP, _VP, _VP, _VP]),
}

_lib = None


def exported_symbols():
    return sorted(_SIGS)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RpccError("librpcc_seg.so is not built (%s); run `python -c 'import __graft_entry__ as g; g.build()'`" % LIB_PATH)
        h = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(h, name)
            fn.restype = res
            fn.argtypes = args
        if h.rpcc_seg_version() != ABI_VERSION:
            raise RpccError("librpcc_seg.so (%s) reports interface version %d, this binding needs %d (stale build: rebuild with "
                            "`python -c 'import __graft_entry__ as g; g.build()'`)" % (LIB_PATH, h.rpcc_seg_version(), ABI_VERSION))
        _lib = h
    return _lib


def check(rc):
    if rc != 0:
        raise RpccError("librpcc_seg: %s (code %d)" % (lib().rpcc_seg_last_error().decode(), rc))
