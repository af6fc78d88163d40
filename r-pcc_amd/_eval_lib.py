"""ctypes binding of librpcc_eval.so (include/rpcc_eval.h), the reconstruction-metrics kernels.  There is no CPU
fallback: if the HIP library is missing, stale or a call fails, this raises."""
import ctypes as C
import os

import torch  # noqa: F401  (imported first so the library binds to the HIP runtime torch already loaded)

from ._lib import RpccError

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "librpcc_eval.so")

ABI_VERSION = 1        # RPCC_EVAL_ABI_VERSION
BRUTEFORCE = 1         # RPCC_EVAL_BRUTEFORCE
KNN = 12               # RPCC_EVAL_KNN
NSUMS = 10             # RPCC_EVAL_NSUMS
MAX_PIXELS = 1 << 26   # RPCC_EVAL_MAX_PIXELS

_VP, _I, _D, _F = C.c_void_p, C.c_int, C.c_double, C.c_float
_SIGS = {
    "rpcc_eval_version": (C.c_int, []),
    "rpcc_eval_last_error": (C.c_char_p, []),
    "rpcc_eval_workspace_bytes": (C.c_size_t, [_I, _I, _I]),
    "rpcc_eval_nn": (C.c_int, [_VP, _VP, _I, _I, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "rpcc_eval_normals": (C.c_int, [_VP, _I, _I, _I, _D, _I, _VP, _VP, _VP, _VP]),
    "rpcc_eval_metrics": (C.c_int, [_VP, _VP, _I, _I, _I, _VP, _VP, _VP, _F, _VP, _VP, _VP]),
}

_lib = None


def exported_symbols():
    return sorted(_SIGS)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RpccError("librpcc_eval.so is not built (%s); run `python -c 'import __graft_entry__ as g; g.build()'`" % LIB_PATH)
        h = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(h, name)
            fn.restype = res
            fn.argtypes = args
        if h.rpcc_eval_version() != ABI_VERSION:
            raise RpccError("librpcc_eval.so (%s) reports interface version %d, this binding needs %d (stale build: rebuild with "
                            "`python -c 'import __graft_entry__ as g; g.build()'`)" % (LIB_PATH, h.rpcc_eval_version(), ABI_VERSION))
        _lib = h
    return _lib


def check(rc):
    if rc != 0:
        raise RpccError("librpcc_eval: %s (code %d)" % (lib().rpcc_eval_last_error().decode(), rc))
