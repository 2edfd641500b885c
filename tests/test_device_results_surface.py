"""Results that stay on the device - undistorted points written to device memory, inlier masks written to device memory - the part
that needs no device: the new symbols are declared, exported and bound, PL_ABI_VERSION is still 5, the ctypes mirrors of the three
new records have the header's layout, every device-free check answers PL_ERR_INVALID with a message that names the cause (before
PL_ERR_NO_DEVICE on a machine without a GPU), and the Python front-ends raise ValueError for what they cannot pass on."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import poselib_amd
from poselib_amd import _lib as L
from poselib_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["pl_undistort_points_dev", "pl_undistort_points_batch_dev", "pl_estimate_dev_masked", "pl_estimate_batch_dev_masked"]
FAR = 0x7F0000001000  # an address nothing dereferences
HAVE_DEVICE = poselib_amd.device_count() > 0
NEEDS_DEVICE = L.PL_ERR_INVALID if HAVE_DEVICE else L.PL_ERR_NO_DEVICE  # (with a device: FAR is no device memory)
OPENCV = api.Camera("OPENCV", [1000.0, 1010.0, 500.0, 505.0, 0.04, -0.015, 8e-4, -6e-4])


def _err():
    return L.lib().pl_last_error().decode()


def test_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "poselib_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(pl_[a-z0-9_]+)\s*\(", text))
    poselib_amd.build()
    lib = L.lib()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in L.EXPORTED_SYMBOLS, name
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is C.c_int, name
    for record in ("pl_device_points_out", "pl_undistort_item_dev", "pl_device_mask"):
        assert record in text, record
    assert re.search(r"#define\s+PL_ABI_VERSION\s+5\b", text) and lib.pl_abi_version() == 5 and L.ABI_VERSION == 5
    for name in ("undistort_points", "undistort_points_batch"):
        assert hasattr(poselib_amd, name), name


LAYOUT_PROGRAM = r"""
#include <stddef.h>
#include <stdio.h>
#include "poselib_amd.h"
#define F(T, m) printf(#T "." #m " %zu\n", offsetof(T, m))
int main(void) {
    printf("pl_device_points_out %zu\npl_undistort_item_dev %zu\npl_device_mask %zu\n", sizeof(pl_device_points_out),
           sizeof(pl_undistort_item_dev), sizeof(pl_device_mask));
    F(pl_device_points_out, data); F(pl_device_points_out, row_stride); F(pl_device_points_out, dtype); F(pl_device_points_out, cols);
    F(pl_undistort_item_dev, status); F(pl_undistort_item_dev, reserved); F(pl_undistort_item_dev, camera);
    F(pl_undistort_item_dev, points2D); F(pl_undistort_item_dev, n); F(pl_undistort_item_dev, out);
    F(pl_device_mask, data); F(pl_device_mask, stride);
    return 0;
}
"""


def test_the_ctypes_mirrors_have_the_headers_layout():
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "layout.c"), os.path.join(tmp, "layout")
        open(src, "w").write(LAYOUT_PROGRAM)
        subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True, capture_output=True)
        lines = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n")
    want = dict((k, int(v)) for k, v in (line.split() for line in lines if line))
    mirrors = {"pl_device_points_out": L.DevicePointsOut, "pl_undistort_item_dev": L.UndistortItemDev, "pl_device_mask": L.DeviceMask}
    assert len(want) == 3 + 4 + 6 + 2
    for name, value in want.items():
        record, _, member = name.partition(".")
        got = getattr(mirrors[record], member).offset if member else C.sizeof(mirrors[record])
        assert got == value, (name, got, value)


# ------------------------------------------------------------------------------------------ un-distortion: the checks without a device
def _src(data=FAR, row_stride=2, dtype=L.PL_F64):
    return L.DevicePoints(data, row_stride, dtype, 2)


def _out(data=FAR + (1 << 20), row_stride=2, dtype=L.PL_F64, cols=2):
    return L.DevicePointsOut(data, row_stride, dtype, cols)


def _undistort(src, out, n=10, cam=OPENCV):
    c = cam._c() if cam is not None else None
    rc = L.lib().pl_undistort_points_dev(None if c is None else C.byref(c), None if src is None else C.byref(src), C.c_size_t(n),
                                         None if out is None else C.byref(out))
    return rc, _err()


BAD_UNDISTORT = {
    "source descriptor is null": (lambda: (None, _out()), "descriptor is null"),
    "destination descriptor is null": (lambda: (_src(), None), "destination: descriptor is null"),
    "source data is null": (lambda: (_src(data=None), _out()), "device points: data is null"),
    "destination data is null": (lambda: (_src(), _out(data=None)), "destination: data is null"),
    "fp32 destination": (lambda: (_src(), _out(dtype=L.PL_F32)), "destination: dtype must be PL_F64"),
    "destination row_stride of 1": (lambda: (_src(), _out(row_stride=1)), "destination: row_stride (elements) is below cols"),
    "misaligned destination": (lambda: (_src(), _out(data=FAR + (1 << 20) + 4)), "destination: data is not aligned"),
    "destination cols": (lambda: (_src(), _out(cols=3)), "destination: cols must be 2"),
    # the source's rows 0 .. 9 span 160 bytes: a destination that starts inside them, or that they start inside
    "partial overlap, destination behind": (lambda: (_src(), _out(data=FAR + 80)), "destination: overlaps the source"),
    "partial overlap, destination in front": (lambda: (_src(), _out(data=FAR - 80)), "destination: overlaps the source"),
    "same address, another stride": (lambda: (_src(), _out(data=FAR, row_stride=4)), "destination: overlaps the source"),
    "same address, fp32 source": (lambda: (_src(dtype=L.PL_F32), _out(data=FAR)), "destination: overlaps the source"),
    "interleaved columns of one block": (lambda: (_src(row_stride=4), _out(data=FAR + 16, row_stride=4)), "destination: overlaps the source"),
}


@pytest.mark.parametrize("case", sorted(BAD_UNDISTORT))
def test_undistort_dev_refuses_a_bad_descriptor_before_the_device(case):
    make, cause = BAD_UNDISTORT[case]
    rc, msg = _undistort(*make())
    assert rc == L.PL_ERR_INVALID and cause in msg, (rc, msg)


def test_undistort_dev_refuses_too_many_rows_before_the_device():
    for n in (1 << 31, (1 << 31) + 5, 1 << 40):
        rc, msg = _undistort(_src(), _out(data=FAR + (1 << 50)), n=n)
        assert rc == L.PL_ERR_INVALID and "too many correspondences" in msg, (n, rc, msg)


def test_undistort_dev_accepts_what_is_allowed_and_then_asks_for_the_device():
    for src, out in ((_src(), _out()),                               # apart
                     (_src(), _out(data=FAR + 160)),                 # ranges that touch
                     (_src(), _out(data=FAR - 160)),
                     (_src(), _out(data=FAR)),                       # in place
                     (_src(row_stride=5), _out(data=FAR, row_stride=5))):
        rc, msg = _undistort(src, out)
        assert rc == NEEDS_DEVICE, (rc, msg)
        assert "overlaps" not in msg
    # n == 0: nothing is read or written, data may be null - only the device itself is asked for, as by pl_undistort_points
    rc, msg = _undistort(_src(data=None), _out(data=None), n=0)
    assert rc == (L.PL_OK if HAVE_DEVICE else L.PL_ERR_NO_DEVICE), (rc, msg)


def test_undistort_dev_takes_the_cameras_of_the_host_form():
    bad = [None, api.Camera("NULL", []), api.Camera("OPENCV", [1000.0, 1000.0, 500.0])]  # (too few parameters)
    unknown = api.Camera("PINHOLE", [1.0, 1.0, 0.0, 0.0])
    for cam in bad:
        rc, msg = _undistort(_src(), _out(), cam=cam)
        assert rc == L.PL_ERR_UNSUPPORTED and "camera model not supported" in msg, (rc, msg)
    c = unknown._c()
    c.model_id = 77
    s, o = _src(), _out()
    assert L.lib().pl_undistort_points_dev(C.byref(c), C.byref(s), 10, C.byref(o)) == L.PL_ERR_UNSUPPORTED
    # ... and says what pl_undistort_points says
    host = np.zeros((4, 2))
    assert L.lib().pl_undistort_points(C.byref(c), host.ctypes.data, 4, host.ctypes.data) == L.PL_ERR_UNSUPPORTED
    assert _err() == _undistort(_src(), _out(), cam=bad[1])[1]
    for model, params in (("SIMPLE_PINHOLE", [800.0, 400.0, 300.0]), ("RADIAL_FISHEYE", [800.0, 400.0, 300.0, 0.01, 0.001])):
        assert _undistort(_src(), _out(), cam=api.Camera(model, params))[0] == NEEDS_DEVICE


def test_the_undistort_batch_names_the_item_that_is_bad():
    lib = L.lib()
    cam = OPENCV._c()
    items = (L.UndistortItemDev * 3)()
    for i, it in enumerate(items):
        it.camera = C.pointer(cam)
        it.points2D, it.n, it.out = _src(data=FAR + i * (1 << 22)), 100, _out(data=FAR + i * (1 << 22) + (1 << 21))
        it.status = 99
    items[1].out = _out(data=FAR + (1 << 22) + (1 << 21), dtype=L.PL_F32)
    assert lib.pl_undistort_points_batch_dev(items, 3) == L.PL_ERR_INVALID
    msg = _err()
    if HAVE_DEVICE:  # (every address here is host memory to a device: the call reports its FIRST failing item)
        assert "item 0:" in msg, msg
    else:
        assert "item 1:" in msg and "destination: dtype must be PL_F64" in msg, msg
    assert items[1].status == L.PL_ERR_INVALID
    assert [items[0].status, items[2].status] == [NEEDS_DEVICE] * 2
    # a camera the stage does not take fails its own item
    null = api.Camera("NULL", [])._c()
    items[1].out = _out(data=FAR + (1 << 22) + (1 << 21))
    items[2].camera = C.pointer(null)
    rc = lib.pl_undistort_points_batch_dev(items, 3)
    assert items[2].status == L.PL_ERR_UNSUPPORTED and rc in (L.PL_ERR_UNSUPPORTED, NEEDS_DEVICE)
    if not HAVE_DEVICE:
        assert rc == L.PL_ERR_UNSUPPORTED and "item 2:" in _err() and "camera model not supported" in _err()
    assert lib.pl_undistort_points_batch_dev(None, 0) == L.PL_OK
    assert lib.pl_undistort_points_batch_dev(None, 2) == L.PL_ERR_INVALID


# ------------------------------------------------------------------------------------------ masks: the checks without a device
def _masked(kind, mask, n=100, scores=False, a=None):
    lib = L.lib()
    o = L.RobustOptions()
    lib.pl_default_robust_options(C.byref(o), kind)
    cam = api.Camera("SIMPLE_PINHOLE", [1000.0, 500.0, 500.0])._c()
    cb = 3 if kind == 0 else 2
    a = a or L.DevicePoints(FAR, 2, L.PL_F64, 2)
    b = L.DevicePoints(FAR + (1 << 30), cb, L.PL_F64, cb)
    sc = L.DeviceScores(FAR + (2 << 30), 1, L.PL_F32, 0, -np.inf)
    model, st, used = np.zeros(9), L.RansacStats(), C.c_size_t(7)
    rc = lib.pl_estimate_dev_masked(kind, C.byref(a), C.byref(b), C.byref(sc) if scores else None, n, C.byref(o),
                                    C.byref(cam) if kind < 2 else None, C.byref(cam) if kind == 1 else None, model.ctypes.data,
                                    None if mask is None else C.byref(mask), C.byref(st), C.byref(used))
    return rc, _err()


@pytest.mark.parametrize("kind", range(4))
@pytest.mark.parametrize("scores", [False, True])
def test_the_masked_call_checks_its_destination_before_the_device(kind, scores):
    rc, msg = _masked(kind, None, scores=scores)
    assert rc == L.PL_ERR_INVALID and "device mask: descriptor is null" in msg, msg
    rc, msg = _masked(kind, L.DeviceMask(None, 1), scores=scores)
    assert rc == L.PL_ERR_INVALID and "device mask: data is null" in msg, msg
    for stride in (0, -1):
        rc, msg = _masked(kind, L.DeviceMask(FAR + (3 << 30), stride), scores=scores)
        assert rc == L.PL_ERR_INVALID and "device mask: stride (bytes) is below 1" in msg, msg
    rc, msg = _masked(kind, L.DeviceMask(FAR + (3 << 30), 1), n=1 << 31, scores=scores)
    assert rc == L.PL_ERR_INVALID and "too many correspondences" in msg, msg
    # the points' own checks still speak, first
    rc, msg = _masked(kind, L.DeviceMask(FAR + (3 << 30), 0), scores=scores, a=L.DevicePoints(FAR, 1, L.PL_F64, 2))
    assert rc == L.PL_ERR_INVALID and "device points" in msg, msg
    # a plausible call: the device is asked for
    rc, msg = _masked(kind, L.DeviceMask(FAR + (3 << 30), 2), scores=scores)
    assert rc == NEEDS_DEVICE, msg


def test_the_masked_call_refuses_what_the_plain_call_refuses():
    assert _masked(7, L.DeviceMask(FAR, 1))[0] == L.PL_ERR_INVALID
    lib = L.lib()
    o = L.RobustOptions()
    lib.pl_default_robust_options(C.byref(o), 0)
    o.estimate_focal_length = 1
    cam = api.Camera("SIMPLE_PINHOLE", [1000.0, 500.0, 500.0])._c()
    a, b, m = L.DevicePoints(FAR, 2, L.PL_F64, 2), L.DevicePoints(FAR, 3, L.PL_F64, 3), L.DeviceMask(FAR, 0)
    pose, st = L.CameraPose(), L.RansacStats()
    rc = lib.pl_estimate_dev_masked(0, C.byref(a), C.byref(b), None, 50, C.byref(o), C.byref(cam), None, C.byref(pose), C.byref(m),
                                    C.byref(st), None)
    assert rc == L.PL_ERR_UNSUPPORTED and "estimate_focal_length" in _err()


def test_the_masked_batch_names_the_item_whose_mask_is_bad():
    lib = L.lib()
    count, n = 3, 50
    items, masks, used = (L.BatchItemDev * count)(), (L.DeviceMask * count)(), (C.c_size_t * count)()
    keep = []
    for i, it in enumerate(items):
        o = L.RobustOptions()
        lib.pl_default_robust_options(C.byref(o), 3)
        model, st, inl = np.zeros(9), L.RansacStats(), np.zeros(n, dtype=np.uint8)
        it.kind, it.n = 3, n
        it.a, it.b = L.DevicePoints(FAR, 2, L.PL_F64, 2), L.DevicePoints(FAR, 2, L.PL_F64, 2)
        it.opt, it.model, it.inliers, it.stats = C.pointer(o), model.ctypes.data, inl.ctypes.data, C.pointer(st)
        keep.append((o, model, st, inl))
        masks[i] = L.DeviceMask(FAR + (1 << 30), 1)
    masks[1] = L.DeviceMask(FAR + (1 << 30), 0)
    masks[2] = L.DeviceMask(None, 0)  # (no data: an item with its host mask, whatever else the entry says)
    assert lib.pl_estimate_batch_dev_masked(items, None, masks, used, count, 4) == L.PL_ERR_INVALID
    msg = _err()
    if HAVE_DEVICE:
        assert "item 0:" in msg and "device points" in msg, msg
    else:
        assert "item 1:" in msg and "device mask: stride (bytes) is below 1" in msg, msg
    assert items[1].status == L.PL_ERR_INVALID
    assert [items[0].status, items[2].status] == [NEEDS_DEVICE] * 2
    assert lib.pl_estimate_batch_dev_masked(None, None, None, None, 0, 4) == L.PL_OK


# ------------------------------------------------------------------------------------------ Python
class FakeDeviceArray:
    """__cuda_array_interface__ over a numpy buffer, whose address stands in for a device address; nothing dereferences it"""

    def __init__(self, array):
        self.array = array
        self.shape = array.shape

    @property
    def __cuda_array_interface__(self):
        a = self.array
        return {"shape": a.shape, "typestr": a.dtype.str, "data": (a.__array_interface__["data"][0], False),
                "strides": None if a.flags.c_contiguous else tuple(a.strides), "version": 3}


def test_python_builds_the_mask_descriptors_and_raises_for_what_it_cannot_pass_on():
    t = np.zeros((3, 40, 5), dtype=np.float32)
    flags = np.zeros((3, 40, 2), dtype=np.bool_)
    base = flags.__array_interface__["data"][0]
    problems = [("hom", FakeDeviceArray(t[i, :, :2]), FakeDeviceArray(t[i, :, 2:4]),
                 {"ransac": {"seed": i}, "inliers_out": FakeDeviceArray(flags[i, :, 1])} if i != 1 else None) for i in range(3)]
    b = api.Batch(problems)
    assert b.on_device and b.masked and not b.scored
    for i in (0, 2):
        assert (b.masks[i].data, b.masks[i].stride) == (base + i * 80 + 1, 2)
    assert not b.masks[1].data and b.mask_out[1] is None and b.mask_out[0] is problems[0][3]["inliers_out"]
    dev = (FakeDeviceArray(t[0, :, :2]), FakeDeviceArray(t[0, :, 2:4]))
    with pytest.raises(ValueError):  # host points with inliers_out
        api.estimate_homography(np.zeros((40, 2)), np.zeros((40, 2)), inliers_out=FakeDeviceArray(flags[0, :, 0]))
    with pytest.raises(ValueError):
        api.Batch([("hom", np.zeros((40, 2)), np.zeros((40, 2)), {"inliers_out": FakeDeviceArray(flags[0, :, 0])})])
    with pytest.raises(ValueError):  # device points, a host mask
        api.estimate_homography(*dev, inliers_out=np.zeros(40, dtype=bool))
    with pytest.raises(ValueError):  # the wrong size
        api.estimate_fundamental(*dev, inliers_out=FakeDeviceArray(flags[0, :30, 0]))
    with pytest.raises(ValueError):  # two-dimensional
        api.estimate_homography(*dev, inliers_out=FakeDeviceArray(flags[0]))
    with pytest.raises(ValueError):  # no one-byte elements
        api.estimate_homography(*dev, inliers_out=FakeDeviceArray(np.zeros(40, dtype=np.int32)))


def test_python_undistort_raises_for_what_it_cannot_pass_on():
    t = np.zeros((40, 4), dtype=np.float64)
    t32 = np.zeros((40, 4), dtype=np.float32)
    cam = OPENCV
    with pytest.raises(ValueError):  # a device array that is no torch tensor needs out=
        api.undistort_points(cam, FakeDeviceArray(t32[:, :2]))
    with pytest.raises(ValueError):  # fp32 output is not offered
        api.undistort_points(cam, FakeDeviceArray(t[:, :2]), out=FakeDeviceArray(t32[:, 2:4]))
    with pytest.raises(ValueError):  # another length
        api.undistort_points(cam, FakeDeviceArray(t[:, :2]), out=FakeDeviceArray(np.zeros((30, 2))))
    with pytest.raises(ValueError):  # a host destination for device points
        api.undistort_points(cam, FakeDeviceArray(t[:, :2]), out=np.zeros((40, 2)))
    with pytest.raises(ValueError):  # out= with host points
        api.undistort_points(cam, np.zeros((40, 2)), out=FakeDeviceArray(np.zeros((40, 2))))
    with pytest.raises(ValueError):  # a column stride of 2
        api.undistort_points(cam, FakeDeviceArray(t[:, :2]), out=FakeDeviceArray(np.zeros((40, 4))[:, ::2]))
    with pytest.raises(ValueError):  # host and device items mixed
        api.undistort_points_batch([(cam, np.zeros((40, 2)), None), (cam, FakeDeviceArray(t[:, :2]), FakeDeviceArray(np.zeros((40, 2))))])
    assert api.undistort_points_batch([]) == []
    # what can be passed on reaches the library: interleaved columns of one block overlap (PL_ERR_INVALID, no device needed)
    with pytest.raises(poselib_amd.PoseLibAmdError, match="overlaps the source"):
        api.undistort_points(cam, FakeDeviceArray(t[:, :2]), out=FakeDeviceArray(t[:, 2:4]))


# ------------------------------------------------------------------------------------------ the range arithmetic under a sanitizer
def test_the_range_arithmetic_under_address_and_undefined_behaviour_sanitizers():
    """poselib_amd/csrc/pl_ranges.h - extents of strided rows, overlap of two byte ranges - is plain host code: a stand-alone program
    with its own main (tests/hostcheck_device_results), built with -fsanitize=address,undefined, runs it over n = 0, stride x n
    overflow, ranges that touch, identical ranges, and every small case against a byte map"""
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "ranges_check")
        src = os.path.join(ROOT, "tests", "hostcheck_device_results", "ranges_check.cc")
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                        src], check=True, capture_output=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ranges_check ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
