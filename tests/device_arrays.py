"""Arrays in device memory for the tests of the *_dev entry points: allocated through the HIP runtime the product library itself
loaded, exposed through __cuda_array_interface__, sliceable like the numpy array they mirror.

Why not torch tensors in the test process: torch ships a HIP runtime of its own.  A process that loads the product library first
and torch afterwards - what a whole-suite run does - holds two runtimes, and memory of one is not an allocation the other knows
(the library then answers PL_ERR_INVALID, as it must).  tests/device_points_torch_child.py covers torch tensors in a process that
imports torch first, which is the order of a program whose matches come from torch."""
import ctypes as C

import numpy as np

from poselib_amd import _lib as L

_hip = None


def hip():
    """the HIP runtime of the product library (the loader hands out the copy that is already in the process)"""
    global _hip
    if _hip is None:
        L.lib()
        h = C.CDLL("libamdhip64.so.7")
        h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        h.hipMallocManaged.argtypes = [C.POINTER(C.c_void_p), C.c_size_t, C.c_uint]
        h.hipHostMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t, C.c_uint]
        h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        h.hipFree.argtypes = [C.c_void_p]
        h.hipHostFree.argtypes = [C.c_void_p]
        h.hipSetDevice.argtypes = [C.c_int]
        _hip = h
    return _hip


class Allocation:
    """kind: "device" (hipMalloc), "managed" (hipMallocManaged), "pinned" (hipHostMalloc)"""

    def __init__(self, nbytes, kind="device"):
        self.kind = kind
        p = C.c_void_p()
        if kind == "device":
            rc = hip().hipMalloc(C.byref(p), max(nbytes, 8))
        elif kind == "managed":
            rc = hip().hipMallocManaged(C.byref(p), max(nbytes, 8), 1)  # hipMemAttachGlobal
        else:
            rc = hip().hipHostMalloc(C.byref(p), max(nbytes, 8), 0)
        assert rc == 0 and p.value, (kind, rc)
        self.ptr = p.value

    def __del__(self):
        try:
            (hip().hipHostFree if self.kind == "pinned" else hip().hipFree)(self.ptr)
        except Exception:
            pass


class DeviceArray:
    """A view into a device allocation that mirrors a numpy array: same shape, dtype, strides and offset."""

    def __init__(self, view, host_base, allocation):
        self.view, self.host_base, self.allocation = view, host_base, allocation

    @classmethod
    def upload(cls, array, dtype=None):
        array = np.ascontiguousarray(array, dtype=dtype)
        alloc = Allocation(array.nbytes)
        if array.nbytes:
            assert hip().hipMemcpy(alloc.ptr, array.ctypes.data, array.nbytes, 1) == 0  # hipMemcpyHostToDevice, synchronous
        return cls(array, array.ctypes.data, alloc)

    def __getitem__(self, index):
        return DeviceArray(self.view[index], self.host_base, self.allocation)

    @property
    def shape(self):
        return self.view.shape

    @property
    def data_ptr(self):
        return self.allocation.ptr + (self.view.__array_interface__["data"][0] - self.host_base)

    @property
    def __cuda_array_interface__(self):
        v = self.view
        return {"shape": v.shape, "typestr": v.dtype.str, "data": (self.data_ptr, False),
                "strides": None if v.flags.c_contiguous else tuple(v.strides), "version": 3}

    def contiguous(self):
        return DeviceArray.upload(self.view)


def on_gpu(x, dtype=None):
    return DeviceArray.upload(x, dtype)


def column_view(x, dtype):
    """columns 1 : 1 + d of an (N, 5) buffer whose other elements are NaN: row stride 5, an offset pointer and, in fp32, an
    address that is not 8-byte aligned"""
    n, d = x.shape
    buf = np.full((n, 5), np.nan, dtype=dtype)
    buf[:, 1:1 + d] = x
    return DeviceArray.upload(buf)[:, 1:1 + d]


def row_view(x, dtype):
    """every second row of a (2 N, d) buffer, NaN between"""
    n, d = x.shape
    buf = np.full((2 * n, d), np.nan, dtype=dtype)
    buf[::2] = x
    return DeviceArray.upload(buf)[::2]
