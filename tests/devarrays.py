"""Moving test arrays to the backend under test and back: "emu" = the emulated build, whose device memory is host memory (numpy arrays pass
through); "hip" = the product library (torch tensors on the current CUDA device)."""
import numpy as np
import pytest

BACKENDS = [pytest.param("emu"), pytest.param("hip", marks=pytest.mark.gpu)]


@pytest.fixture
def lib(request, backend):
    """the library of a test parametrised over BACKENDS"""
    return request.getfixturevalue("emu_lib" if backend == "emu" else "hip_lib")


def to_dev_plain(a, backend):
    """a plain (unstructured) array as it is; None stays None"""
    if backend == "emu" or a is None:
        return a
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def to_dev(a, backend):
    """a record array as the bytes of its records, [..., itemsize] uint8 (torch has no structured dtypes); a uint8 array as it is"""
    if backend == "emu" or a is None:
        return a
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(a.shape + (-1,) if a.dtype.names else a.shape)).cuda()


def uploader(backend):
    """to_dev_plain with the backend bound: the `to_dev` argument of LbaWindows, InertialWindows and the pose optimisations"""
    return lambda a: to_dev_plain(a, backend)


def to_host(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def bits(rec):
    """the bytes of float records with every NaN made the same: x86 and the GPU produce different NaN payloads (0/0 of a point at depth +-0),
    the reference's comparisons do not see the payload"""
    rec = np.array(rec, copy=True)
    for name in rec.dtype.names:
        if rec.dtype[name] == np.float32:
            rec[name][np.isnan(rec[name])] = np.float32(np.nan)
    return rec.view(np.uint8)
