"""ctypes binding of tests/hostmath_tangent/libhostmath_tangent.so - a TEST-ONLY host compilation of the tangent-Sampson path of the
device headers (un-projection with its Jacobian, exact score and mask, refiner, fp32 pre-filter).  Built on first use; never used
by the product."""
from __future__ import annotations

import ctypes as C
import glob
import os
import subprocess

import numpy as np

from hostmath_lib import CameraParams, LMOptions, camera_params, lm_options  # noqa: F401  (the records are the device's)

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostmath_tangent")
_LIB = os.path.join(_DIR, "libhostmath_tangent.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        csrc = os.path.join(os.path.dirname(_DIR), "..", "poselib_amd", "csrc")
        srcs = [os.path.join(_DIR, "hostmath_tangent.cc"), os.path.join(_DIR, "Makefile")] + glob.glob(os.path.join(csrc, "pl_*.h"))
        if not os.path.exists(_LIB) or any(os.path.getmtime(s) > os.path.getmtime(_LIB) for s in srcs):
            subprocess.check_call(["make", "-C", _DIR, "-s", "-B", "libhostmath_tangent.so"])
        _lib = C.CDLL(_LIB)
        _lib.tg_score.restype = C.c_double
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def cam_of(cam):
    """CameraParams of a camera dict {"model": id, "params": [...]}; None: the identity camera"""
    return camera_params() if cam is None else camera_params(int(cam["model"]), list(cam["params"]))


def unproject_with_jac(cam, pix):
    """d (n, 3), M (n, 6), ok (n,) of camera_unproject_with_jac"""
    pix = _f64(pix).reshape(-1, 2)
    n = pix.shape[0]
    d, M, ok = np.zeros((n, 3)), np.zeros((n, 6)), np.zeros(max(n, 1), dtype=np.uint8)
    c = cam_of(cam)
    lib().tg_unproject_with_jac(C.byref(c), _p(pix), C.c_uint32(n), _p(d), _p(M), _p(ok))
    return d, M, ok[:n].astype(bool)


def score(pose, d1, d2, M1, M2, max_error):
    """(score, count, mask, r2) as k_score_seq<EST_RELT> / k_mask<EST_RELT> evaluate them"""
    d1, d2, M1, M2, pose = _f64(d1), _f64(d2), _f64(M1), _f64(M2), _f64(pose)
    n = d1.shape[0]
    cnt = C.c_uint64(0)
    mask, r2 = np.zeros(max(n, 1), dtype=np.uint8), np.zeros(max(n, 1))
    s = lib().tg_score(_p(pose), _p(d1), _p(d2), _p(M1), _p(M2), C.c_uint32(n), C.c_double(max_error * max_error), C.byref(cnt), _p(mask),
                       _p(r2))
    return float(s), int(cnt.value), mask[:n].astype(bool), r2[:n]


def refine(pose, d1, d2, M1, M2, opt: LMOptions, mask=None):
    """(pose, iterations, initial cost, cost) of the LM loop with Refiner<EST_RELT>"""
    d1, d2, M1, M2 = _f64(d1), _f64(d2), _f64(M1), _f64(M2)
    p = _f64(pose).copy()
    it = C.c_uint32(0)
    costs = np.zeros(2)
    m8 = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    lib().tg_refine(_p(d1), _p(d2), _p(M1), _p(M2), C.c_uint32(d1.shape[0]), _p(p), C.byref(opt), None if m8 is None else _p(m8),
                    C.byref(it), _p(costs))
    return p, int(it.value), float(costs[0]), float(costs[1])


def prefilter(E, d1, d2, M1, M2, max_error):
    """(status, rejected, below, r2): the fp32 pre-filter of k_score_tangent and the exact r^2 < thr^2 for the 3x3 matrix E"""
    d1, d2, M1, M2 = _f64(d1), _f64(d2), _f64(M1), _f64(M2)
    E = _f64(np.asarray(E).reshape(9))
    n = d1.shape[0]
    rej, below, r2 = np.zeros(max(n, 1), dtype=np.uint8), np.zeros(max(n, 1), dtype=np.uint8), np.zeros(max(n, 1))
    st = lib().tg_prefilter(_p(E), _p(d1), _p(d2), _p(M1), _p(M2), C.c_uint32(n), C.c_double(max_error * max_error), _p(rej), _p(below),
                            _p(r2))
    return int(st), rej[:n].astype(bool), below[:n].astype(bool), r2[:n]
