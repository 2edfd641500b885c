"""pl_atan2 and pl_tan (poselib_amd/csrc/pl_libm.h) against the host's libm (glibc 2.35 in this image), BIT FOR BIT: the very
header hipcc compiles is compiled for the host (tests/hostmath_trig) next to the host's own atan2 / tan.  Both restate the variant
glibc selects on hosts with FMA (__ieee754_atan2_fma, __tan_fma); on a host without FMA libm takes another code path and the last
bit may differ, as for acos / cos (tests/test_libm_vs_glibc.py).

Arguments: 2e7 per function from the streams of hostmath_trig.cc (log-uniform magnitudes over 120 binades and over the whole exponent
range, both signs of x and of y, what the fisheye cameras send, ratios around the switches of the algorithm), the 129 doubles around
every branch threshold of the restatement, and for tan the doubles nearest to n pi / 2 inside the domain."""
import math

import numpy as np
import pytest

import hostmath_trig_lib as T


def _has_fma():
    try:
        return " fma " in open("/proc/cpuinfo").read()
    except OSError:
        return True


pytestmark = pytest.mark.skipif(not _has_fma(), reason="host without FMA: glibc runs its sse2 variants of atan2 / tan here")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def test_atan2_is_bit_identical_to_glibc_on_2e7_arguments():
    bad, first = T.mismatches("atan2", 20_000_000, 5)
    assert bad == 0, (bad, first[0].hex(), first[1].hex())
    y, x = T.args("atan2", 200_000, 5)  # the stream is what it says: both signs of x, mostly positive y, 120 binades and more
    assert (x < 0).mean() > 0.4 and (x > 0).mean() > 0.4 and 0.6 < (y > 0).mean() < 0.9
    assert np.log2(np.abs(x)).min() < -900 and np.log2(np.abs(x)).max() > 900
    assert np.isfinite(x).all() and np.isfinite(y).all() and (y != 0).all()


def test_tan_is_bit_identical_to_glibc_on_2e7_arguments():
    bad, first = T.mismatches("tan", 20_000_000, 6)
    assert bad == 0, (bad, first[0].hex())
    x, _ = T.args("tan", 200_000, 6)
    assert np.abs(x).max() <= 25.0 and (np.abs(x) <= 4.0).mean() > 0.5 and (x < 0).mean() > 0.2
    assert np.abs(x)[np.abs(x) > 0].min() < 1e-10


def test_atan2_around_every_branch_threshold_and_in_every_quadrant():
    y, x = T.atan2_edges()
    assert y.size > 50_000
    got, want = T.pl("atan2", y, x), T.glibc("atan2", y, x)
    bad = np.flatnonzero(bits(got) != bits(want))
    assert bad.size == 0, (bad.size, y[bad[:3]], x[bad[:3]])
    # each branch is reached: exponent difference beyond +-57, scaled operands, both polynomial and table, x = 0
    de = np.floor(np.log2(np.abs(y))) - np.floor(np.log2(np.where(x == 0, 1.0, np.abs(x))))
    u = np.minimum(np.abs(y), np.abs(x)) / np.maximum(np.abs(y), np.abs(x))
    assert (de >= 57).any() and (de <= -57).any() and (np.abs(x) < 2.0 ** -500).any() and (np.abs(y) > 2.0 ** 500).any()
    assert (u < 0.0625).any() and (u >= 0.0625).any() and (x == 0).any() and (np.abs(y) == np.abs(x)).any()
    assert want[(x == 0) & (y > 0)].tolist() == [math.pi / 2] * int(((x == 0) & (y > 0)).sum())


def test_tan_around_every_branch_threshold_and_the_multiples_of_half_pi():
    x = T.tan_edges()
    assert x.size > 20_000 and np.abs(x).max() == 25.0
    got, want = T.pl("tan", x), T.glibc("tan", x)
    bad = np.flatnonzero(bits(got) != bits(want))
    assert bad.size == 0, (bad.size, [v.hex() for v in x[bad[:3]]])
    for n in range(1, 16):  # the double nearest to n pi / 2 is among them (n * fl(pi / 2) rounds to it or its neighbour)
        assert (np.abs(np.abs(x) - n * math.pi / 2) <= 2 * np.spacing(n * math.pi / 2)).any(), n
    assert np.abs(want).max() > 1e15  # (tan next to pi / 2: the -cot branch's double-double reciprocal)


def test_outside_the_domain_the_result_is_finite_or_follows_glibc_on_specials():
    big = np.array([25.000000000000004, -26.0, 1e3, -1e8, 1e22, 1.7e308])
    out = T.pl("tan", big)
    assert np.isfinite(out).all() and np.abs(out - T.glibc("tan", big)).max() <= 1e-9 * np.abs(out).max()
    assert np.isnan(T.pl("tan", np.array([np.inf, -np.inf, np.nan]))).all()
    y = np.array([0.0, -0.0, 0.0, np.inf, 1.0, np.nan, 1.0])
    x = np.array([1.0, -1.0, -0.0, 1.0, -np.inf, 1.0, np.nan])
    got, want = T.pl("atan2", y, x), T.glibc("atan2", y, x)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.allclose(got[~np.isnan(got)], want[~np.isnan(want)], rtol=1e-15, atol=0)
