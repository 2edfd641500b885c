"""ctypes binding of tests/hostmath_bound/libhostmath_bound.so - a TEST-ONLY host compilation of the bound tier's per-pair function
(pl_prefilter.h pf_abs_r2_lower).  Built on first use; never used by the product."""
from __future__ import annotations

import ctypes as C
import glob
import os
import subprocess

import numpy as np

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostmath_bound")
_LIB = os.path.join(_DIR, "libhostmath_bound.so")
_lib = None
SCALE = 1 << 20  # kPfBoundScale: quanta per thr^2


def lib():
    global _lib
    if _lib is None:
        csrc = os.path.join(os.path.dirname(_DIR), "..", "poselib_amd", "csrc")
        srcs = [os.path.join(_DIR, "hostmath_bound.cc"), os.path.join(_DIR, "Makefile")] + glob.glob(os.path.join(csrc, "pl_*.h"))
        if not os.path.exists(_LIB) or any(os.path.getmtime(s) > os.path.getmtime(_LIB) for s in srcs):
            subprocess.check_call(["make", "-C", _DIR, "-s", "-B", "libhostmath_bound.so"])
        _lib = C.CDLL(_LIB)
    return _lib


def bound(rec, cols, thr2, xy_absmax, residual=True):
    """(enabled, L (n,) float32, maybe (n,) bool, quanta (n,) uint32) of a model record (hostmath_lib.pose_record) against the
    correspondences cols = (x, y, X, Y, Z); residual: the second stage's bound (pf_abs_r2_lower), else the first stage's verdict"""
    arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in cols]
    ptrs = (C.c_void_p * 5)(*[a.ctypes.data for a in arrs])
    n = arrs[0].shape[0]
    L = np.zeros(max(n, 1), dtype=np.float32)
    maybe = np.zeros(max(n, 1), dtype=np.uint8)
    q = np.zeros(max(n, 1), dtype=np.uint32)
    rec = np.ascontiguousarray(rec, dtype=np.float64)
    en = lib().hb_bound(C.c_int(1 if residual else 0), rec.ctypes.data_as(C.c_void_p), ptrs, C.c_uint32(n), C.c_double(thr2), C.c_float(xy_absmax),
                        L.ctypes.data_as(C.c_void_p), maybe.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.c_void_p))
    return bool(en), L[:n], maybe[:n].astype(bool), q[:n]
