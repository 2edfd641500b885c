"""Correspondences from device memory, the part that needs no device: the *_dev entry points are declared, exported and bound;
every plain rejection of a pl_device_points descriptor comes back as PL_ERR_INVALID before the device is touched; the Python
binding turns a __cuda_array_interface__ object into the descriptor the library expects.  No compute calls are made here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import poselib_amd
from poselib_amd import _lib as L
from poselib_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DEV_SYMBOLS = ["pl_estimate_absolute_pose_dev", "pl_estimate_relative_pose_dev", "pl_estimate_fundamental_dev",
               "pl_estimate_homography_dev", "pl_problem_create_dev", "pl_problem_create_tangent_dev",
               "pl_debug_check_device_points", "pl_debug_point_stats_dev"]


def test_dev_entry_points_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "poselib_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(pl_[a-z0-9_]+)\s*\(", text))
    poselib_amd.build()
    lib = L.lib()
    for name in DEV_SYMBOLS:
        assert name in declared, name
        assert name in L.EXPORTED_SYMBOLS, name
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is C.c_int, name  # (a signature was declared in _lib._declare)
    assert "pl_device_points" in text and re.search(r"#define\s+PL_F32\s+1", text) and re.search(r"#define\s+PL_F64\s+0", text)
    assert re.search(r"#define\s+PL_ABI_VERSION\s+5\b", text) and lib.pl_abi_version() == 5
    # the descriptor's layout: pointer, int64, int32, int32
    assert C.sizeof(L.DevicePoints) == 24 and L.DevicePoints.row_stride.offset == 8 and L.DevicePoints.cols.offset == 20


def _desc(data=0x7F0000001000, row_stride=2, dtype=L.PL_F64, cols=2):
    return L.DevicePoints(data, row_stride, dtype, cols)


PLAIN_REJECTIONS = {
    "null descriptor": (None, 10, 2),
    "null data with n > 0": (_desc(data=None), 10, 2),
    "cols 3 where 2 is expected": (_desc(cols=3, row_stride=3), 10, 2),
    "cols 2 where 3 is expected": (_desc(), 10, 3),
    "row_stride below cols": (_desc(row_stride=1), 10, 2),
    "negative row_stride": (_desc(row_stride=-2), 10, 2),
    "unknown dtype": (_desc(dtype=2), 10, 2),
    "fp64 data at an odd address": (_desc(data=0x7F0000001001), 10, 2),
    "fp64 data aligned to 4 only": (_desc(data=0x7F0000001004), 10, 2),
    "fp32 data aligned to 2 only": (_desc(data=0x7F0000001002, dtype=L.PL_F32), 10, 2),
    "n beyond 2^31 - 1": (_desc(), 1 << 31, 2),
}


@pytest.mark.parametrize("case", sorted(PLAIN_REJECTIONS))
def test_plain_rejections_come_before_the_device(case):
    """PL_ERR_INVALID - not PL_ERR_NO_DEVICE - on a machine without a GPU: the check ran before get_context"""
    desc, n, cols = PLAIN_REJECTIONS[case]
    assert api.check_device_points(desc, n, cols) == L.PL_ERR_INVALID, case
    assert L.lib().pl_last_error()  # (a message names the cause)


def test_an_empty_set_passes_without_a_device():
    assert api.check_device_points(_desc(data=None), 0, 2) == L.PL_OK
    assert api.check_device_points(_desc(data=None, dtype=L.PL_F32, cols=3, row_stride=7), 0, 3) == L.PL_OK


@pytest.mark.skipif(poselib_amd.device_count() > 0, reason="GPU present")
def test_a_plausible_descriptor_needs_the_device():
    assert api.check_device_points(_desc(), 10, 2) == L.PL_ERR_NO_DEVICE


@pytest.mark.skipif(poselib_amd.device_count() > 0, reason="GPU present")
def test_entry_points_reject_before_the_device():
    """the entry points themselves: a bad descriptor is PL_ERR_INVALID where a good one would be PL_ERR_NO_DEVICE"""
    lib = L.lib()
    o = L.RobustOptions()
    lib.pl_default_robust_options(C.byref(o), 2)
    st, F = L.RansacStats(), np.zeros(9)
    good, bad = _desc(), _desc(row_stride=1)
    h = C.c_void_p()
    assert lib.pl_estimate_fundamental_dev(C.byref(good), C.byref(bad), 100, C.byref(o), F.ctypes.data, None, C.byref(st)) == L.PL_ERR_INVALID
    assert lib.pl_estimate_fundamental_dev(C.byref(good), C.byref(good), 100, C.byref(o), F.ctypes.data, None, C.byref(st)) == L.PL_ERR_NO_DEVICE
    assert lib.pl_problem_create_dev(2, C.byref(bad), C.byref(good), 100, C.byref(h)) == L.PL_ERR_INVALID
    assert lib.pl_problem_create_dev(0, C.byref(good), C.byref(good), 100, C.byref(h)) == L.PL_ERR_INVALID  # (points3D: cols 3)
    assert lib.pl_problem_create_tangent_dev(C.byref(good), None, 100, None, None, C.byref(h)) == L.PL_ERR_INVALID
    # below the estimator's minimum: the host form's default stats, nothing touched
    st.iterations = 7
    assert lib.pl_estimate_fundamental_dev(C.byref(good), C.byref(good), 6, C.byref(o), F.ctypes.data, None, C.byref(st)) == L.PL_OK
    assert st.iterations == 0 and st.model_score == np.finfo(np.float64).max
    assert lib.pl_estimate_homography_dev(C.byref(good), C.byref(good), 3, C.byref(o), F.ctypes.data, None, C.byref(st)) == L.PL_OK
    # estimate_focal_length is not served from device memory
    lib.pl_default_robust_options(C.byref(o), 0)
    o.estimate_focal_length = 1
    cam, pose = api.Camera("SIMPLE_PINHOLE", [1000.0, 500.0, 500.0])._c(), L.CameraPose()
    p3 = _desc(cols=3, row_stride=3)
    assert lib.pl_estimate_absolute_pose_dev(C.byref(good), C.byref(p3), 100, C.byref(o), C.byref(cam), C.byref(pose), None,
                                             C.byref(st)) == L.PL_ERR_UNSUPPORTED


class FakeDeviceArray:
    """What a GPU array library hands out: __cuda_array_interface__ (version 3) - here over a numpy buffer, whose address stands in
    for a device address; nothing dereferences it."""

    def __init__(self, array, with_contiguous=True, strides="auto"):
        self.array = array
        self.with_contiguous = with_contiguous
        self.strides = strides

    @property
    def __cuda_array_interface__(self):
        a = self.array
        strides = (None if a.flags.c_contiguous else tuple(a.strides)) if self.strides == "auto" else self.strides
        return {"shape": a.shape, "typestr": a.dtype.str, "data": (a.__array_interface__["data"][0], False), "strides": strides,
                "version": 3}

    def __getattr__(self, name):
        if name == "contiguous" and self.with_contiguous:
            return lambda: FakeDeviceArray(np.ascontiguousarray(self.array))
        raise AttributeError(name)


@pytest.mark.parametrize("dtype,code,size", [(np.float64, L.PL_F64, 8), (np.float32, L.PL_F32, 4)])
def test_descriptor_of_views(dtype, code, size):
    buf = np.arange(40 * 5, dtype=dtype).reshape(40, 5)
    base = buf.__array_interface__["data"][0]
    # contiguous
    whole = np.ascontiguousarray(buf[:, :2])
    d, n, _ = api._device_points(FakeDeviceArray(whole), 2)
    assert (d.data, d.row_stride, d.dtype, d.cols, n) == (whole.__array_interface__["data"][0], 2, code, 2, 40)
    # columns 1:3 of the (N, 5) buffer: byte strides -> ELEMENTS, the view's offset in `data`
    d, n, _ = api._device_points(FakeDeviceArray(buf[:, 1:3]), 2)
    assert (d.data, d.row_stride, d.dtype, d.cols, n) == (base + size, 5, code, 2, 40)
    d, n, _ = api._device_points(FakeDeviceArray(buf[:, 2:5]), 3)
    assert (d.data, d.row_stride, d.cols, n) == (base + 2 * size, 5, 3, 40)
    # every second row
    d, n, _ = api._device_points(FakeDeviceArray(buf[::2, 1:3]), 2)
    assert (d.data, d.row_stride, n) == (base + size, 10, 20)
    # an explicit strides tuple of a contiguous array
    d, n, _ = api._device_points(FakeDeviceArray(whole, strides=(2 * size, size)), 2)
    assert (d.row_stride, n) == (2, 40)
    # nothing to read: a null pointer, whatever the object says
    d, n, _ = api._device_points(FakeDeviceArray(buf[:0, 1:3]), 2)
    assert (d.data, n) == (None, 0)


def test_descriptor_rejects_other_dtypes_and_shapes():
    for dtype in (np.float16, np.int32, np.int64, np.uint8):
        with pytest.raises(ValueError):
            api._device_points(FakeDeviceArray(np.zeros((8, 2), dtype=dtype)), 2)
    with pytest.raises(ValueError):
        api._device_points(FakeDeviceArray(np.zeros((8, 3))), 2)
    with pytest.raises(ValueError):
        api._device_points(FakeDeviceArray(np.zeros(8)), 2)
    with pytest.raises(ValueError):  # byte strides that are no multiple of the element
        api._device_points(FakeDeviceArray(np.zeros((8, 2)), strides=(20, 8)), 2)


def test_column_stride_other_than_one_is_made_contiguous_on_the_device():
    wide = np.arange(64, dtype=np.float32).reshape(8, 8)
    view = wide[:, ::3][:, :2]  # column stride 3
    d, n, owner = api._device_points(FakeDeviceArray(view), 2)
    assert isinstance(owner, FakeDeviceArray) and owner.array.flags.c_contiguous  # (the object's own .contiguous())
    assert (d.data, d.row_stride, n) == (owner.array.__array_interface__["data"][0], 2, 8)
    assert np.array_equal(owner.array, view)
    transposed = np.arange(16, dtype=np.float64).reshape(2, 8).T  # (8, 2), column stride 8
    d, n, owner = api._device_points(FakeDeviceArray(transposed), 2)
    assert d.row_stride == 2 and np.array_equal(owner.array, transposed)
    with pytest.raises(ValueError):  # no way to make it contiguous without leaving the device
        api._device_points(FakeDeviceArray(view, with_contiguous=False), 2)


def test_host_and_device_points_do_not_mix():
    host = np.zeros((8, 2))
    with pytest.raises(ValueError):
        api._Points(FakeDeviceArray(np.zeros((8, 2))), host, 2, 2)
    with pytest.raises(ValueError):
        api._Points(host, FakeDeviceArray(np.zeros((8, 2))), 2, 2)
    with pytest.raises(ValueError):  # different lengths
        api._Points(FakeDeviceArray(np.zeros((8, 2))), FakeDeviceArray(np.zeros((9, 2))), 2, 2)
    p = api._Points(FakeDeviceArray(np.zeros((8, 2))), FakeDeviceArray(np.zeros((8, 3), dtype=np.float32)), 2, 3)
    assert p.on_device and p.n == 8
    p = api._Points(host, [[0.0, 1.0]] * 8, 2, 2)  # host arrays and lists: today's path
    assert not p.on_device and p.n == 8
