"""ctypes binding of libpswin_poly_hip.so (include/pswin_poly.h), the polygon rasteriser's own library.  As with _lib there is no
fallback: if the library is missing or a call fails, this raises."""
import ctypes
import os

from ._lib import PswinError, check, stream_of

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "libpswin_poly_hip.so")
ABI_VERSION = 1

_vp, _i = ctypes.c_void_p, ctypes.c_int

# name -> argtypes; every function returns int.  Mirrors include/pswin_poly.h one to one.
_PROTOTYPES = {
    "pswin_poly_version": [],
    "pswin_poly_workspace": [_i, _i, _i, _i, _vp],
    "pswin_poly_masks": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp],
}

_lib = None


def exported_symbols():
    return sorted(_PROTOTYPES)


def load():
    """Load the library once; raise loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise PswinError(f"{LIB_PATH} is missing: build it with `python -m panoswintransformerobjectdetection_amd.build` (hipcc, gfx950).  "
                         "The polygon kernels have no CPU or PyTorch fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, argtypes in _PROTOTYPES.items():
        fn = getattr(lib, name)          # AttributeError if the .so does not export a declared symbol
        fn.argtypes = argtypes
        fn.restype = ctypes.c_int
    v = lib.pswin_poly_version()
    if v != ABI_VERSION:
        raise PswinError(f"libpswin_poly_hip.so ABI {v} != expected {ABI_VERSION}; rebuild")
    _lib = lib
    return lib


def call(name, ref_tensor, *args):
    """Invoke an entry point on the current stream of ref_tensor's device and raise on a non-zero status."""
    import torch
    lib = load()
    with torch.cuda.device(ref_tensor.device):
        rc = getattr(lib, name)(*args, stream_of(ref_tensor))
    check(rc, name)
