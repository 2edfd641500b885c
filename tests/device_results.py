"""Device memory that the library WRITES, for the tests of the entry points whose results stay on the GPU (undistorted points,
inlier masks): an allocation filled with a sentinel, views into it like tests/device_arrays.py makes them, and a download that
shows every byte - the ones the call had to write and the ones it had to leave alone."""
import ctypes as C

import numpy as np

from device_arrays import DeviceArray, hip


def sentinel_array(shape, dtype, fill):
    """a device array of `shape` whose every element is `fill`; slice it for the destination view"""
    return DeviceArray.upload(np.full(shape, fill, dtype=dtype))


def download(arr):
    """the WHOLE allocation behind a DeviceArray as a numpy array shaped like the array it was uploaded from (views download
    their base, so the bytes around a view can be checked); synchronous.  The array must have been uploaded from an array that
    owns its data (np.full, np.array, ...), not from a view of a larger host array."""
    base = arr.view if arr.view.base is None else arr.view.base
    while base.base is not None:
        base = base.base
    out = np.empty_like(base)
    if out.nbytes:
        h = hip()
        h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        assert h.hipMemcpy(out.ctypes.data, arr.allocation.ptr, out.nbytes, 2) == 0  # hipMemcpyDeviceToHost
    return out


def bits(a):
    """float64 values as their bit patterns: NaN equals NaN, -0.0 differs from 0.0"""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
