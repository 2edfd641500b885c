"""The device's pl_atan2 and pl_tan, bit for bit, in the code that runs on the GPU (pl_debug_device_math2), against the host's
glibc on the streams and threshold neighbourhoods of the CPU test (tests/test_libm_trig_vs_glibc.py, tests/hostmath_trig_lib.py).
4e6 arguments per function from the streams (the CPU test walks 2e7 of the same generator through the host compile of the same
header), every branch threshold with 64 doubles on either side, for tan the doubles nearest to n pi / 2 inside the domain."""
import numpy as np
import pytest

import hostmath_trig_lib as T

pytestmark = pytest.mark.gpu

N_STREAM = 4_000_000


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def test_device_atan2_is_bit_identical_to_glibc(gpu):
    y, x = T.args("atan2", N_STREAM, 5)
    ey, ex = T.atan2_edges()
    y, x = np.r_[y, ey], np.r_[x, ex]
    got = gpu.device_math2(0, y, x)  # (the entry's first array is atan2's first argument)
    want = T.glibc("atan2", y, x)
    bad = np.flatnonzero(bits(got) != bits(want))
    print("atan2: arguments", y.size, "mismatches", bad.size)
    assert bad.size == 0, (bad.size, [(y[i].hex(), x[i].hex(), got[i].hex(), want[i].hex()) for i in bad[:3]])
    assert (x < 0).any() and (x == 0).any() and (y < 0).any()


def test_device_tan_is_bit_identical_to_glibc_inside_its_domain(gpu):
    x = np.r_[T.args("tan", N_STREAM, 6)[0], T.tan_edges()]
    assert np.abs(x).max() == 25.0
    got = gpu.device_math2(1, x)
    want = T.glibc("tan", x)
    bad = np.flatnonzero(bits(got) != bits(want))
    print("tan: arguments", x.size, "mismatches", bad.size)
    assert bad.size == 0, (bad.size, [(x[i].hex(), got[i].hex(), want[i].hex()) for i in bad[:3]])


def test_outside_the_domains_results_are_finite_and_unknown_codes_are_rejected(gpu):
    big = np.array([25.000000000000004, -26.0, 1e3, -1e8, 1e22, 1.7e308])
    out = gpu.device_math2(1, big)
    assert np.isfinite(out).all() and np.abs(out - T.glibc("tan", big)).max() <= 1e-9 * np.abs(out).max()
    assert np.isnan(gpu.device_math2(1, np.array([np.inf, -np.inf, np.nan]))).all()
    y = np.array([0.0, -0.0, 0.0, np.inf, 1.0, np.nan])
    x = np.array([1.0, -1.0, -0.0, 1.0, -np.inf, 1.0])
    got, want = gpu.device_math2(0, y, x), T.glibc("atan2", y, x)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.allclose(got[~np.isnan(got)], want[~np.isnan(want)], rtol=1e-15, atol=0)
    assert gpu.device_math2(0, np.zeros(0), np.zeros(0)).size == 0
    for fn in (-1, 2, 12):
        with pytest.raises(gpu.PoseLibAmdError):
            gpu.device_math2(fn, np.ones(4), np.ones(4))
    with pytest.raises(gpu.PoseLibAmdError):
        gpu.device_math2(0, np.ones(4))  # atan2 without its second array
