"""ctypes binding of liborbhip.so (C ABI in include/orbhip.h, mirrored in _abi.py) and the array helpers every wrapper module uses.

There is NO fallback: if the hipcc-built library is missing or fails to load, importing callers get an
OrbHipError.  (Build it with tools/build_lib.sh or __graft_entry__.build().)"""
import ctypes as C
import os

import numpy as np

from ._abi import (KP_DTYPE, ORB_E_ABORTED, ORB_E_CAPACITY, ORB_E_EMPTY_IMAGE, ORB_E_HIP, ORB_E_INVALID, ORB_E_NOMEM, ORB_OK,  # noqa: F401
                   PROTOTYPES, OrbxConfig)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ORBHIP_LIB", os.path.join(_HERE, "liborbhip.so"))   # explicit override for kernel experiments


class OrbHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("orbhip error %d: %s" % (code, msg))
        self.code = code


def bind(lib, prototypes=PROTOTYPES):
    """Declare the prototypes on a loaded CDLL, once per library object."""
    if not getattr(lib, "_orbhip_bound", False):
        for name, (res, args) in prototypes.items():
            fn = getattr(lib, name)  # AttributeError if the symbol is missing: loud by design
            fn.restype = res
            fn.argtypes = args
        lib._orbhip_bound = True
    return lib


_lib = None


def load():
    """Load the product library.  Raises OrbHipError if it is absent — there is no CPU path."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OrbHipError(ORB_E_INVALID, "%s not found: build it with tools/build_lib.sh (hipcc, gfx950); "
                              "there is no CPU fallback" % LIB_PATH)
        # One HIP runtime per process: the PyTorch wheel bundles its own libamdhip64; if liborbhip.so is dlopen'ed first it binds the system copy
        # and torch later loads a second runtime whose device pointers the first one rejects (every launch fails with ORB_E_HIP).  Importing torch
        # first makes the library's libamdhip64 dependency resolve to the copy that is already mapped.
        try:
            import torch  # noqa: F401
        except Exception:   # noqa: BLE001  (the library itself does not need torch)
            pass
        _lib = bind(C.CDLL(LIB_PATH))
    return _lib


# ---- array helpers: arrays are torch CUDA tensors (product path) or numpy arrays (emulated test build, whose "device" is host memory) ----------
def ptr(a):
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        assert a.flags["C_CONTIGUOUS"]
        return C.c_void_p(a.ctypes.data)
    assert a.is_contiguous()
    return C.c_void_p(a.data_ptr())


def zeros(like, shape, dtype):
    """like: a numpy array or None -> numpy zeros; a torch tensor or a torch device -> torch zeros there (uint16 as int16 bit patterns)."""
    if like is None or isinstance(like, np.ndarray):
        return np.zeros(shape, dtype)
    import torch
    tdt = {np.uint8: torch.uint8, np.uint16: torch.int16, np.int32: torch.int32, np.int64: torch.int64, np.float32: torch.float32,
           np.float64: torch.float64}[dtype]
    return torch.zeros(shape, dtype=tdt, device=getattr(like, "device", like))


def stream(like):
    """torch's current stream on the device of `like` (a tensor or a torch device); None (the default stream) for numpy arrays."""
    if like is None or isinstance(like, np.ndarray):
        return None
    import torch
    return C.c_void_p(torch.cuda.current_stream(getattr(like, "device", like)).cuda_stream)


def to_host(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def check(rc, what):
    if rc != 0:
        raise OrbHipError(rc, what)


def check_capacity(bad, message):
    """The raise of the host-side overflow checks: bad = host indices of the entries that overflowed, message(first of them) -> text."""
    if len(bad):
        raise OrbHipError(ORB_E_CAPACITY, message(int(bad[0])))
