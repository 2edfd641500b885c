"""Shared-focal relative pose and 1D-radial absolute pose from device memory (pl_estimate_shared_focal_relative_pose_dev,
pl_estimate_1D_radial_absolute_pose_dev) - the part that needs no device: the symbols are declared with the documented argument
order, exported and bound, every descriptor mistake is PL_ERR_INVALID with a message that names the cause (before
PL_ERR_NO_DEVICE on a machine without a GPU) for points, scores and mask alike, what the host forms answer without a launch the
device forms answer the same way, and the Python front-ends raise ValueError for what they cannot pass on."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import poselib_amd
from poselib_amd import _lib as L
from poselib_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAR = 0x7F0000001000  # an address nothing dereferences
HAVE_DEVICE = poselib_amd.device_count() > 0
NEEDS_DEVICE = L.PL_ERR_INVALID if HAVE_DEVICE else L.PL_ERR_NO_DEVICE  # (with a device: FAR is no device memory)
SFOCAL, RADIAL = "pl_estimate_shared_focal_relative_pose_dev", "pl_estimate_1D_radial_absolute_pose_dev"
START = [0.5, 0.5, -0.5, 0.5, 0.25, -2.0, 3.0]


def _err():
    return L.lib().pl_last_error().decode()


def _header():
    return open(os.path.join(ROOT, "include", "poselib_amd.h")).read()


def test_symbols_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    poselib_amd.build()
    lib = L.lib()
    for name in (SFOCAL, RADIAL, "pl_debug_point_stats_about_dev"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is C.c_int, name
    for name in (SFOCAL, "pl_debug_point_stats_about_dev"):  # (the 1D names are outside the lower-case pattern of that list)
        assert name in L.EXPORTED_SYMBOLS, name
    # new symbols, no record changed: the layout version stays
    assert re.search(r"#define\s+PL_ABI_VERSION\s+5\b", text) and lib.pl_abi_version() == 5 and L.ABI_VERSION == 5
    assert hasattr(poselib_amd, "point_stats_about_dev")


def _arguments(name):
    """the parameter names of a declaration of the header, in order"""
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    body = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
    return [re.search(r"(\w+)\s*$", part.strip()).group(1) for part in body.split(",")]


def test_the_documented_argument_order():
    assert _arguments(SFOCAL) == ["x1", "x2", "scores", "n", "pp", "opt", "pose", "focal", "inliers", "mask", "stats", "n_used"]
    assert _arguments(RADIAL) == ["points2D", "points3D", "scores", "n", "opt", "pose", "inliers", "mask", "stats", "n_used"]
    assert _arguments("pl_debug_point_stats_about_dev") == ["x1", "x2", "n", "cx", "cy", "out"]
    P = C.POINTER
    lib = L.lib()
    assert getattr(lib, SFOCAL).argtypes[:4] == [P(L.DevicePoints), P(L.DevicePoints), P(L.DeviceScores), C.c_size_t]
    assert getattr(lib, SFOCAL).argtypes[9:] == [P(L.DeviceMask), P(L.RansacStats), P(C.c_size_t)]
    assert getattr(lib, RADIAL).argtypes[:4] == [P(L.DevicePoints), P(L.DevicePoints), P(L.DeviceScores), C.c_size_t]
    assert getattr(lib, RADIAL).argtypes[7:] == [P(L.DeviceMask), P(L.RansacStats), P(C.c_size_t)]


# ------------------------------------------------------------------------------------------ the calls, on addresses nothing reads
def _points(cols, data=FAR, row_stride=None, dtype=L.PL_F64):
    return L.DevicePoints(data, cols if row_stride is None else row_stride, dtype, cols)


def _scores(data=FAR + (2 << 30), stride=1, dtype=L.PL_F32, min_score=-np.inf):
    return L.DeviceScores(data, stride, dtype, 0, min_score)


def _mask(data=FAR + (3 << 30), stride=1):
    return L.DeviceMask(data, stride)


def _options(kind=1):
    o = L.RobustOptions()
    L.lib().pl_default_robust_options(C.byref(o), kind)
    return o


def _pose():
    p = L.CameraPose()
    for i in range(4):
        p.q[i] = START[i]
    for i in range(3):
        p.t[i] = START[4 + i]
    return p


def _ref(x):
    return None if x is None else C.byref(x)


def call(which, a="default", b="default", scores=None, mask=None, n=100, opt="default", pose="default", pp="default", focal="default"):
    """-> (rc, message, pose as a list, stats, n_used)"""
    lib = L.lib()
    radial = which == "radial"
    a = _points(2) if a == "default" else a
    b = _points(3 if radial else 2, data=FAR + (1 << 30)) if b == "default" else b
    opt = _options(0 if radial else 1) if opt == "default" else opt
    pose = _pose() if pose == "default" else pose
    st, used = L.RansacStats(), C.c_size_t(7)
    st.iterations, st.num_inliers, st.model_score = 99, 99, 99.0
    if radial:
        rc = lib.pl_estimate_1D_radial_absolute_pose_dev(_ref(a), _ref(b), _ref(scores), n, _ref(opt), _ref(pose), None, _ref(mask),
                                                         C.byref(st), C.byref(used))
    else:
        ppa = np.array([500.0, 500.0]) if pp == "default" else pp
        f = C.c_double(1.0) if focal == "default" else focal
        rc = lib.pl_estimate_shared_focal_relative_pose_dev(_ref(a), _ref(b), _ref(scores), n, None if ppa is None else ppa.ctypes.data,
                                                            _ref(opt), _ref(pose), _ref(f), None, _ref(mask), C.byref(st), C.byref(used))
    return rc, _err(), (None if pose is None else list(pose.q) + list(pose.t)), st, used.value


BAD = {
    "first set: null descriptor": (dict(a=None), "device points: descriptor is null"),
    "second set: null descriptor": (dict(b=None), "device points: descriptor is null"),
    "first set: cols": (dict(a=_points(3)), "device points: cols must be 2"),
    "first set: dtype": (dict(a=_points(2, dtype=7)), "device points: dtype must be PL_F64 or PL_F32"),
    "first set: row_stride below cols": (dict(a=_points(2, row_stride=1)), "device points: row_stride (elements) is below cols"),
    "first set: misaligned fp64": (dict(a=_points(2, data=FAR + 4)), "device points: data is not aligned"),
    "first set: misaligned fp32": (dict(a=_points(2, data=FAR + 2, dtype=L.PL_F32)), "device points: data is not aligned"),
    "first set: null data": (dict(a=_points(2, data=None)), "device points: data is null"),
    "scores: dtype": (dict(scores=_scores(dtype=5)), "device scores: dtype must be PL_F64 or PL_F32"),
    "scores: stride": (dict(scores=_scores(stride=0)), "device scores: stride (elements) is below 1"),
    "scores: misaligned": (dict(scores=_scores(data=FAR + 2)), "device scores: data is not aligned"),
    "scores: null data": (dict(scores=_scores(data=None)), "device scores: data is null"),
    "scores: NaN min_score": (dict(scores=_scores(min_score=np.nan)), "device scores: min_score is NaN"),
    "mask: stride": (dict(mask=_mask(stride=0)), "device mask: stride (bytes) is below 1"),
    "mask: null data": (dict(mask=_mask(data=None)), "device mask: data is null"),
    "too many rows": (dict(n=1 << 31), "too many correspondences"),
}
SECOND = {  # the second set's own columns
    "sfocal": {"second set: cols": (dict(b=_points(3, data=FAR + (1 << 30))), "device points: cols must be 2"),
               "second set: row_stride below cols": (dict(b=_points(2, data=FAR + (1 << 30), row_stride=1)), "row_stride (elements) is below cols")},
    "radial": {"second set: cols": (dict(b=_points(2, data=FAR + (1 << 30))), "device points: cols must be 3"),
               "second set: row_stride below cols": (dict(b=_points(3, data=FAR + (1 << 30), row_stride=2)), "row_stride (elements) is below cols")},
}


@pytest.mark.parametrize("which", ["sfocal", "radial"])
@pytest.mark.parametrize("case", sorted(BAD) + ["second set: cols", "second set: row_stride below cols"])
def test_a_descriptor_mistake_is_invalid_before_the_device(which, case):
    kw, cause = dict(BAD, **SECOND[which])[case]
    rc, msg, pose, st, used = call(which, **kw)
    assert rc == L.PL_ERR_INVALID and cause in msg, (rc, msg)
    assert pose == START and used == 0


@pytest.mark.parametrize("which", ["sfocal", "radial"])
def test_a_plausible_call_asks_for_the_device(which):
    for kw in (dict(), dict(scores=_scores()), dict(mask=_mask()), dict(scores=_scores(stride=5, dtype=L.PL_F64), mask=_mask(stride=3)),
               dict(a=_points(2, row_stride=5, dtype=L.PL_F32, data=FAR + 4))):
        rc, msg, pose, st, used = call(which, **kw)
        assert rc == NEEDS_DEVICE, (kw, rc, msg)


def test_null_pp_pose_and_focal_are_invalid_as_in_the_host_form():
    lib = L.lib()
    host = np.zeros((10, 2))
    o, p, f, st = _options(), _pose(), C.c_double(1.0), L.RansacStats()
    pp = np.array([500.0, 500.0])
    for kw in (dict(pp=None), dict(pose=None), dict(focal=None)):
        rc, msg, *_ = call("sfocal", **kw)
        assert rc == L.PL_ERR_INVALID and msg == "null argument", (kw, rc, msg)
    # ... what the host entry point says
    assert lib.pl_estimate_shared_focal_relative_pose(host.ctypes.data, host.ctypes.data, 10, None, C.byref(o), C.byref(p), C.byref(f), None,
                                                      C.byref(st)) == L.PL_ERR_INVALID and _err() == "null argument"
    assert lib.pl_estimate_shared_focal_relative_pose(host.ctypes.data, host.ctypes.data, 10, pp.ctypes.data, C.byref(o), None, C.byref(f), None,
                                                      C.byref(st)) == L.PL_ERR_INVALID
    # a null pose of the 1D-radial form, in the host form's words
    rc, msg, *_ = call("radial", pose=None)
    assert rc == L.PL_ERR_INVALID and msg == "points / pose pointer is null", (rc, msg)
    assert lib.pl_estimate_1D_radial_absolute_pose(host.ctypes.data, host.ctypes.data, 10, C.byref(_options(0)), None, None,
                                                   C.byref(st)) == L.PL_ERR_INVALID and _err() == msg


@pytest.mark.parametrize("which", ["sfocal", "radial"])
def test_option_validation_is_the_host_forms(which):
    lib = L.lib()
    host = np.zeros((10, 3))
    for field in ("tangent_sampson", "estimate_focal_length", "estimate_extra_params"):
        o = _options(0 if which == "radial" else 1)
        setattr(o, field, 1)
        rc, msg, pose, st, used = call(which, opt=o)
        assert rc == L.PL_ERR_UNSUPPORTED, (field, rc, msg)
        p, f, hs = _pose(), C.c_double(1.0), L.RansacStats()
        if which == "radial":
            want = lib.pl_estimate_1D_radial_absolute_pose(host.ctypes.data, host.ctypes.data, 10, C.byref(o), C.byref(p), None, C.byref(hs))
        else:
            pp = np.array([500.0, 500.0])
            want = lib.pl_estimate_shared_focal_relative_pose(host.ctypes.data, host.ctypes.data, 10, pp.ctypes.data, C.byref(o), C.byref(p),
                                                              C.byref(f), None, C.byref(hs))
        assert want == rc and _err() == msg
    rc, msg, *_ = call(which, opt=None)
    assert rc == L.PL_ERR_INVALID and "options pointer is null" in msg
    o = _options()
    o.min_fov = np.nan
    rc, msg, *_ = call(which, opt=o)
    assert rc == L.PL_ERR_INVALID and "min_fov is NaN" in msg


def test_radial_with_four_rows_gives_default_stats_without_a_device():
    """the host form's answer for n < 5 (robust.cc:892-895), before any launch: a fake device address is never looked at"""
    for n in (0, 1, 4):
        rc, msg, pose, st, used = call("radial", n=n)
        assert rc == L.PL_OK, (n, rc, msg)
        assert pose == START
        assert (st.iterations, st.refinements, st.num_inliers, st.inlier_ratio, st.model_score, st.hypotheses) == (0, 0, 0, 0.0, 0.0, 0)
    # ... but five rows are read
    assert call("radial", n=5)[0] == NEEDS_DEVICE
    # and the descriptors are still looked at
    rc, msg, *_ = call("radial", n=4, a=_points(3))
    assert rc == L.PL_ERR_INVALID and "cols must be 2" in msg


# ------------------------------------------------------------------------------------------ the Python front-ends
class FakeDeviceArray:
    """looks like device memory to the binding (__cuda_array_interface__); nothing reaches the library in these tests"""

    def __init__(self, shape, typestr="<f8"):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (FAR, False), "strides": None, "version": 3}


def _front_ends():
    host2, host3 = np.zeros((20, 2)), np.zeros((20, 3))
    dev2, dev3 = FakeDeviceArray((20, 2)), FakeDeviceArray((20, 3))
    return [(lambda a, b, **kw: api.estimate_shared_focal_relative_pose(a, b, [500.0, 500.0], None, None, **kw), host2, host2, dev2, dev2),
            (lambda a, b, **kw: api.estimate_1D_radial_absolute_pose(a, b, None, None, **kw), host2, host3, dev2, dev3)]


def test_python_refuses_what_it_cannot_pass_on():
    for fn, ha, hb, da, db in _front_ends():
        with pytest.raises(ValueError, match="one point set is on the GPU"):
            fn(da, hb)
        with pytest.raises(ValueError, match="one point set is on the GPU"):
            fn(ha, db)
        with pytest.raises(ValueError, match="inliers_out= goes with points on the GPU"):
            fn(ha, hb, inliers_out=FakeDeviceArray((20,), "|b1"))
        with pytest.raises(ValueError, match="points and scores must be in the same place"):
            fn(da, db, scores=np.zeros(20))
        with pytest.raises(ValueError, match="points and scores must be in the same place"):
            fn(ha, hb, scores=FakeDeviceArray((20,)))
        with pytest.raises(ValueError, match="min_score without scores"):
            fn(ha, hb, min_score=0.5)
        with pytest.raises(ValueError, match="min_score is NaN"):
            fn(da, db, scores=FakeDeviceArray((20,)), min_score=float("nan"))
        with pytest.raises(ValueError, match="19 scores for 20 correspondences"):
            fn(da, db, scores=FakeDeviceArray((19,)))
        with pytest.raises(ValueError, match="expected 20 elements"):
            fn(da, db, inliers_out=FakeDeviceArray((21,), "|u1"))
        with pytest.raises(ValueError, match="must hold one-byte"):
            fn(da, db, inliers_out=FakeDeviceArray((20,), "<f4"))
