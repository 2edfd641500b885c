"""ctypes binding of tests/hostmath_trig/libhostmath_trig.so - a TEST-ONLY host compilation of pl_atan2 / pl_tan
(poselib_amd/csrc/pl_libm.h) together with the host's own atan2 / tan in a C loop.  Built on first use; never used by the
product."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostmath_trig")
_LIB = os.path.join(_DIR, "libhostmath_trig.so")
FN = {"atan2": 0, "tan": 1}
_lib = None


def lib():
    global _lib
    if _lib is None:
        csrc = os.path.join(os.path.dirname(_DIR), "..", "poselib_amd", "csrc")
        srcs = [os.path.join(_DIR, "hostmath_trig.cc"), os.path.join(_DIR, "Makefile")]
        srcs += [os.path.join(csrc, f) for f in ("pl_libm.h", "pl_libm_tables.h", "pl_defs.h")]
        if not os.path.exists(_LIB) or any(os.path.getmtime(s) > os.path.getmtime(_LIB) for s in srcs):
            subprocess.check_call(["make", "-C", _DIR, "-s", "-B", "libhostmath_trig.so"])
        _lib = C.CDLL(_LIB)
        _lib.ht_mismatches.restype = C.c_uint64
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def args(fn, count, seed):
    """the stream of the bit-for-bit tests: (a, b) = (y, x) for atan2, (x, zeros) for tan"""
    a, b = np.zeros(count), np.zeros(count)
    lib().ht_args(FN[fn], C.c_uint64(seed), C.c_uint64(count), _p(a), _p(b))
    return a, b


def _call(f, fn, a, b):
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.zeros_like(a) if b is None else np.ascontiguousarray(b, dtype=np.float64)
    out = np.zeros_like(a)
    f(FN[fn], _p(a), _p(b), C.c_uint64(a.size), _p(out))
    return out


def glibc(fn, a, b=None):
    """the host's libm in a C loop: atan2(a, b) or tan(a)"""
    return _call(lib().ht_glibc, fn, a, b)


def pl(fn, a, b=None):
    """pl_libm.h compiled for the host: pl_atan2(a, b) or pl_tan(a)"""
    return _call(lib().ht_pl, fn, a, b)


def mismatches(fn, count, seed):
    """(number of arguments of the stream on which pl_* and the host's libm differ in any bit, the first such pair)"""
    bad = np.zeros(2)
    n = lib().ht_mismatches(FN[fn], C.c_uint64(count), C.c_uint64(seed), _p(bad))
    return int(n), (float(bad[0]), float(bad[1]))


def around(v, k=64):
    """the 2 k + 1 doubles around v"""
    base = np.array([v], dtype=np.float64).view(np.int64)[0]
    d = np.arange(-k, k + 1, dtype=np.int64)
    return (base + (d if v >= 0 else -d)).astype(np.int64).view(np.float64)


def atan2_edges():
    """(y, x) around every branch threshold of pl_atan2, in every quadrant"""
    ys, xs = [], []

    def add(y, x):  # y fixed with x's neighbours, x fixed with y's neighbours, both signs of each
        for sy in (1.0, -1.0):
            for sx in (1.0, -1.0):
                nx, ny = around(x), around(y)
                ys.extend([np.full_like(nx, sy * y), sy * ny])
                xs.extend([sx * nx, np.full_like(ny, sx * x)])

    for s in (1.0, 1.5, 1.9999999999):
        add(s * 2.0 ** 57, s)  # the exponent difference 57 (ATAN2_EP): y / x "infinite" ...
        add(s * 2.0 ** 56, s)
        add(s, s * 2.0 ** 57)  # ... and "zero"
        add(s, s * 2.0 ** 56)
    for e in (-500, 500):  # the scaling thresholds
        add(2.0 ** e, 2.0 ** e)
        add(2.0 ** e, 3.0 * 2.0 ** e)
        add(3.0 * 2.0 ** e, 2.0 ** e)
        add(2.0 ** e, 2.0 ** (e + 40))
        add(2.0 ** (e + 40), 2.0 ** e)
    for m in (1.0, 3.0, 1e-3, 7e5):
        add(m, m)  # |y| = |x|
        add(m, 16.0 * m)  # u = 1 / 16 (ATAN2_INV16)
        add(16.0 * m, m)
        for k in (16, 17, 100, 255):  # where the table row changes: u = (k + 1 / 2) / 256
            add(m * (k + 0.5), m * 256.0)
            add(m * 256.0, m * (k + 0.5))
    add(2.0 ** -1022, 1.0)
    add(1.0, 2.0 ** -1022)
    add(2.0 ** 1023, 1.0)
    add(1.0, 2.0 ** 1023)
    y, x = np.concatenate(ys), np.concatenate(xs)
    keep = np.isfinite(y) & np.isfinite(x) & (y != 0)
    y, x = y[keep], x[keep]
    return np.concatenate([y, np.array([1.0, 1.0, -1.0, -1.0, 1e-8, 2.0 ** -1022])]), np.concatenate([x, np.array([0.0, -0.0, 0.0, -0.0, 0.0, -0.0])])


def tan_edges():
    """x around every branch threshold of pl_tan: g1 .. g4, the doubles nearest to n pi / 2 inside the domain, the reduced
    argument around +-g2 and around the changes of the table row"""
    import math

    g1, g2, g3, g4 = (float.fromhex(h) for h in ("0x1.b096cp-27", "0x1.f212dp-5", "0x1.92f1ap-1", "0x1.9p4"))
    pts = [g1, g2, g3, g4]
    pts += [(k + 15.5) / 256 for k in (0, 1, 2, 50, 100, 184, 185, 186)]
    for n in range(1, 16):
        h = n * math.pi / 2  # (n * the double nearest to pi / 2, rounded: within an ulp of the double nearest to n pi / 2)
        pts += [h, h + g2, h - g2, h + g3, h - g3, h + (50 + 15.5) / 256, h - (50 + 15.5) / 256]
    pts = [p for p in pts if p < 25.2]
    xs = [around(p) for p in pts] + [-around(p) for p in pts]
    x = np.concatenate(xs)
    return x[np.abs(x) <= g4]
