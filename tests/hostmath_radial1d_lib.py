"""ctypes binding of tests/hostmath_radial1d/libhostmath_radial1d.so - a TEST-ONLY host compilation of the 1D-radial path of the
device headers (minimal solver, exact score and mask, fp32 pre-filter, refiner).  Built on first use; never used by the product."""
from __future__ import annotations

import ctypes as C
import glob
import os
import subprocess

import numpy as np

from hostmath_lib import LMOptions, lm_options  # noqa: F401  (the records are the device's)

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostmath_radial1d")
_LIB = os.path.join(_DIR, "libhostmath_radial1d.so")
_lib = None


def _sources():
    csrc = os.path.join(os.path.dirname(_DIR), "..", "poselib_amd", "csrc")
    return [os.path.join(_DIR, "hostmath_radial1d.cc"), os.path.join(_DIR, "Makefile")] + glob.glob(os.path.join(csrc, "pl_*.h"))


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB) or any(os.path.getmtime(s) > os.path.getmtime(_LIB) for s in _sources()):
            subprocess.check_call(["make", "-C", _DIR, "-s", "-B", "libhostmath_radial1d.so"])
        _lib = C.CDLL(_LIB)
        _lib.rd_score.restype = C.c_double
    return _lib


def check_program():
    """the stand-alone program of tests/hostmath_radial1d/radial1d_check.cc, built with AddressSanitizer and
    UndefinedBehaviorSanitizer; run as a child process, never loaded into Python"""
    exe = os.path.join(_DIR, "radial1d_check")
    srcs = _sources() + [os.path.join(_DIR, "radial1d_check.cc")]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in srcs):
        subprocess.check_call(["make", "-C", _DIR, "-s", "-B", "radial1d_check"])
    return exe


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a if shape is None else np.ascontiguousarray(a.reshape(shape))


def p5lp_radial(xs, Xs):
    """(counts (S,), poses (S, 4, 7), nan flags (S, 4)) of p5lp_radial_emit per sample"""
    xs, Xs = _f64(xs, (-1, 5, 2)), _f64(Xs, (-1, 5, 3))
    S = xs.shape[0]
    counts, poses, nan = np.zeros(S, dtype=np.uint32), np.zeros((S, 4, 7)), np.zeros((S, 4), dtype=np.uint8)
    lib().rd_p5lp(_p(xs), _p(Xs), C.c_uint32(S), _p(counts), _p(poses), _p(nan))
    return counts.astype(int), poses, nan.astype(bool)


def normalized2(x):
    x = _f64(x, (-1, 2))
    out = np.zeros_like(x)
    lib().rd_normalized2(_p(x), C.c_uint32(x.shape[0]), _p(out))
    return out


def score(pose, x, X, max_error):
    """(score, count, mask) as k_score_seq<EST_RAD1D> / k_mask<EST_RAD1D> evaluate them"""
    x, X, pose = _f64(x, (-1, 2)), _f64(X, (-1, 3)), _f64(pose)
    n = x.shape[0]
    cnt = C.c_uint64(0)
    mask = np.zeros(max(n, 1), dtype=np.uint8)
    s = lib().rd_score(_p(pose), _p(x), _p(X), C.c_uint32(n), C.c_double(max_error * max_error), C.byref(cnt), _p(mask))
    return float(s), int(cnt.value), mask[:n].astype(bool)


def prefilter(pose, x, X, max_error):
    """(status, rejected, inlier): the fp32 pre-filter of k_score_radial1d and the exact decision for a pose"""
    x, X, pose = _f64(x, (-1, 2)), _f64(X, (-1, 3)), _f64(pose)
    n = x.shape[0]
    rej, inl = np.zeros(max(n, 1), dtype=np.uint8), np.zeros(max(n, 1), dtype=np.uint8)
    st = lib().rd_prefilter(_p(pose), _p(x), _p(X), C.c_uint32(n), C.c_double(max_error * max_error), _p(rej), _p(inl))
    return int(st), rej[:n].astype(bool), inl[:n].astype(bool)


def refine(pose, x, X, opt: LMOptions, mask=None):
    """(pose, iterations, initial cost, cost) of the LM loop with Refiner<EST_RAD1D>, every sum in correspondence order"""
    x, X = _f64(x, (-1, 2)), _f64(X, (-1, 3))
    p = _f64(pose).copy()
    it = C.c_uint32(0)
    costs = np.zeros(2)
    m8 = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    lib().rd_refine(_p(x), _p(X), C.c_uint32(x.shape[0]), _p(p), C.byref(opt), None if m8 is None else _p(m8), C.byref(it), _p(costs))
    return p, int(it.value), float(costs[0]), float(costs[1])
