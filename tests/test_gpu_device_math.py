"""The device's scalar math, bit for bit, in the code that actually runs on the GPU (pl_debug_device_math).

Parity with the reference rests on a few primitives compiled by hipcc for gfx950: pl_libm.h's restatements of glibc's
cbrt / acos / cos / sin / sincos (the cubic solvers of P3P and the 7-point solver, quat_exp of every LM step), IEEE sqrt and
division, the Nielsen update's cube (pl_refine.h lm_cube: an FMA form on the device only) and the fp16 conversions of the
matrix-core pre-filters (pl_prefilter.h: conversion instructions on the device only).  test_libm_vs_glibc.py and
test_prefilter_property.py check a host compile of the same headers; here the device evaluates the same argument streams
(hostmath hm_math_args) plus the neighbourhood of every branch threshold - for each threshold t and -t, the 64 doubles on
either side - and the results are compared with the host's glibc, with numpy's IEEE arithmetic and with numpy's float16."""
import math
from fractions import Fraction

import numpy as np
import pytest

import hostmath_lib as HM

pytestmark = pytest.mark.gpu

MAX_CALL = 1 << 25  # values per pl_debug_device_math call (the entry takes up to 2^28)
COS_DOMAIN_HI = 0x419921FB  # |x| < 105414350: cos and sincos are glibc's (pl_libm.h)
SIN_DOMAIN_HI = 0x400368FD  # |x| < 2.426265: sin is glibc's
HP0 = float.fromhex("0x1.921FB54442D18p0")  # pi / 2 in two parts (pl_libm.h kHp0, kHp1)
HP1 = float.fromhex("0x1.1A62633145C07p-54")


def _device(gpu, fn, x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    parts = [gpu.device_math(fn, x[i:i + MAX_CALL]) for i in range(0, x.size, MAX_CALL)]
    return np.concatenate(parts) if parts else x.copy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _from_bits(b):
    return np.ascontiguousarray(b, dtype=np.uint64).view(np.float64)


def _hi(words):
    """the doubles whose high word is `words` (low word 0): the thresholds as pl_libm.h writes them"""
    return _from_bits(np.asarray(words, dtype=np.uint64) << np.uint64(32))


def _near(ts, k=64):
    """t and -t for every t in ts, each with the k doubles on either side (no NaN patterns)"""
    b = _bits(np.abs(np.asarray(ts, dtype=np.float64))).astype(np.int64)
    b = (b[:, None] + np.arange(-k, k + 1)).ravel()
    b = np.unique(b[(b >= 0) & (b <= 0x7FF0000000000000)]).astype(np.uint64)
    return np.r_[_from_bits(b), -_from_bits(b)]


def _powers_of_two():
    return np.ldexp(1.0, np.arange(-1074, 1024))


def _high_word(x):
    return (_bits(x) >> np.uint64(32)).astype(np.uint32) & np.uint32(0x7FFFFFFF)


def _halfpi_multiples(nmax=10**6, k=4):
    """the doubles nearest n pi / 2, 1 <= n <= nmax, both signs, +-k ulps: n times pi / 2 in three parts, the first two
    products exact, so the sum is within one ulp of n pi / 2 - the window is widened by that ulp"""
    n = np.arange(1, nmax + 1, dtype=np.float64)
    p1 = float(_from_bits(_bits(np.array([HP0])) & np.uint64(~((1 << 21) - 1) & 0xFFFFFFFFFFFFFFFF))[0])  # 32 bits
    p2 = HP0 - p1  # exact, 21 bits
    return _near((n * p1 + n * p2) + n * HP1, k + 1)


def _log_uniform(rs, lo, hi, count):
    """both signs, magnitudes log-uniform in [lo, hi)"""
    v = np.exp(rs.uniform(math.log(lo), math.log(hi), count))
    return v * rs.choice([-1.0, 1.0], count)


def _report(name, x, bad, got, want):
    n = int(bad.sum())
    print(f"{name}: {n} mismatches of {x.size}")
    if not n:
        return ""
    i = int(np.flatnonzero(bad)[0])
    return (f"{name}: {n} mismatches of {x.size}; first argument {float(x[i]).hex()}: device {int(got[i]):#018x} "
            f"reference {int(want[i]):#018x}")


def _assert_bitwise(name, x, got, want):
    """every bit equal; a NaN equals any NaN"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    bad = (_bits(got) != _bits(want)) & ~(np.isnan(got) & np.isnan(want))
    msg = _report(name, x, bad, _bits(got), _bits(want))
    assert not msg, msg


def _assert_outside_domain(name, x, got, want):
    """outside the stated domain only finiteness is promised; the agreement with glibc is printed"""
    fin = np.isfinite(x)
    assert np.isfinite(got[fin]).all(), (name, float(x[fin][~np.isfinite(got[fin])][0]).hex())
    same = (_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want))
    print(f"{name} outside its domain: {x.size} arguments, {100.0 * (1.0 - same.mean()):.3f} % differ from glibc")


def _glibc_fma_host():
    # glibc selects its FMA variants of acos / cos / sin on hosts with FMA - the variant pl_libm.h restates
    try:
        return " fma " in open("/proc/cpuinfo").read()
    except OSError:
        return True


def test_unknown_function_code_is_rejected(gpu):
    x = np.ones(4)
    for fn in (-1, 12, 1000):
        with pytest.raises(gpu.PoseLibAmdError):
            gpu.device_math(fn, x)


def test_cbrt_matches_glibc(gpu):
    modes = [HM.math_args("cbrt", count, 11 + mode, mode)
             for mode, count in ((0, 3_000_000), (1, 4_000_000), (2, 4_000_000), (3, 1_000_000))]  # test_libm_vs_glibc.py
    k = np.arange(1, 2**17 + 1, dtype=np.float64) ** 3  # exact
    cubes = np.r_[k, np.nextafter(k, 0), np.nextafter(k, np.inf)]
    tiny, dmin, dmax = 5e-324, 2.0**-1022, np.finfo(np.float64).max
    special = np.array([0.0, np.inf, np.nan, tiny, dmin - tiny, dmin, dmax])
    p2 = _powers_of_two()
    x = np.r_[np.concatenate(modes), special, -special, cubes, -cubes, _near(np.r_[0.0, dmin, dmax, np.inf, p2])]
    _assert_bitwise("cbrt", x, _device(gpu, 3, x), HM.glibc("cbrt", x))


def test_acos_matches_glibc(gpu):
    if not _glibc_fma_host():
        pytest.skip("host without FMA: glibc runs its sse2 variant of acos here")
    thresholds = np.array([2.0**-55, 1 / 8, 1 / 4, 1 / 2, 3 / 4, 0.921875, 0.953125, 31 / 32, 1.0])
    # the start of every interval of the asin table (pl_acos: widths 2^15, 2^14, 2^13 in the high word)
    starts = _hi(np.r_[np.arange(0x3FC00000, 0x3FD00000, 1 << 15), np.arange(0x3FD00000, 0x3FE00000, 1 << 14),
                       np.arange(0x3FE00000, 0x3FF00000, 1 << 13)])
    rs = np.random.RandomState(6)
    above = np.r_[1.0 + rs.uniform(0, 1, 10_000), 2.0, 1e300, np.inf, np.nan]
    x = np.r_[HM.math_args("acos", 20_000_000, 3), _near(thresholds), _near(starts, 4), above, -above]
    _assert_bitwise("acos", x, _device(gpu, 6, x), HM.glibc("acos", x))


def _cos_arguments(rs):
    thresholds = np.r_[2.0**-27, _hi([0x3FEB6000, 0x400368FD, COS_DOMAIN_HI])]
    odd = np.arange(1, 2.43 * 256, 2) / 256  # kBig + |x| rounds to multiples of 2^-7: ties at the odd multiples of 2^-8
    outside = np.r_[_log_uniform(rs, 105414350.0, 1e300, 100_000), np.inf, -np.inf, np.nan]
    return np.r_[_near(thresholds), _near(odd, 1), _halfpi_multiples(), outside]


def test_cos_matches_glibc_inside_its_domain(gpu):
    if not _glibc_fma_host():
        pytest.skip("host without FMA: glibc runs its sse2 variant of cos here")
    x = np.r_[HM.math_args("cos", 15_000_000, 4), _cos_arguments(np.random.RandomState(4))]
    got, want = _device(gpu, 4, x), HM.glibc("cos", x)
    inside = _high_word(x) < COS_DOMAIN_HI
    _assert_bitwise("cos", x[inside], got[inside], want[inside])
    _assert_outside_domain("cos", x[~inside], got[~inside], want[~inside])


def test_sin_matches_glibc_inside_its_domain(gpu):
    if not _glibc_fma_host():
        pytest.skip("host without FMA: glibc runs its sse2 variant of sin here")
    rs = np.random.RandomState(5)
    thresholds = np.r_[2.0**-26, 0.126, _hi([0x3FEB6000, SIN_DOMAIN_HI])]
    outside = np.r_[_log_uniform(rs, 2.426265, 1e300, 100_000), np.inf, -np.inf, np.nan]
    x = np.r_[HM.math_args("sin", 15_000_000, 5), _near(thresholds), outside]
    got, want = _device(gpu, 5, x), HM.glibc("sin", x)
    inside = _high_word(x) < SIN_DOMAIN_HI
    _assert_bitwise("sin", x[inside], got[inside], want[inside])
    _assert_outside_domain("sin", x[~inside], got[~inside], want[~inside])


def test_sincos_matches_glibc_inside_its_domain(gpu):
    """quat_exp's pair: one sincos() call in the reference's build (pl_libm.h pl_sincos), both outputs"""
    x = np.r_[HM.math_args("sincos", 20_000_000, 11), _near([0.126]), _cos_arguments(np.random.RandomState(7))]
    sn, cs = _device(gpu, 7, x), _device(gpu, 8, x)
    want_sn, want_cs = HM.glibc("sincos", x)
    inside = _high_word(x) < COS_DOMAIN_HI
    _assert_bitwise("sincos: sine", x[inside], sn[inside], want_sn[inside])
    _assert_bitwise("sincos: cosine", x[inside], cs[inside], want_cs[inside])
    _assert_outside_domain("sincos: sine", x[~inside], sn[~inside], want_sn[~inside])
    _assert_outside_domain("sincos: cosine", x[~inside], cs[~inside], want_cs[~inside])


def test_sqrt_is_ieee(gpu):
    rs = np.random.RandomState(1)
    binades = _from_bits(rs.randint(1, 0x7FF0000000000000, 5_000_000, dtype=np.uint64))
    subnormal = _from_bits(rs.randint(1, 1 << 52, 1_000_000, dtype=np.uint64))
    # exact squares: y with at most 26 significant bits (y^2 exact and normal) and the squares' neighbours
    y = np.ldexp(rs.randint(1 << 25, 1 << 26, 1_000_000).astype(np.float64), rs.randint(-536, 486, 1_000_000))
    sq = y * y
    negative = np.r_[-_from_bits(rs.randint(1, 0x7FF0000000000000, 500_000, dtype=np.uint64)), -np.inf, -5e-324]
    x = np.r_[binades, subnormal, sq, np.nextafter(sq, 0), np.nextafter(sq, np.inf), negative,
              0.0, -0.0, np.inf, np.nan, _near(_powers_of_two())]
    with np.errstate(invalid="ignore"):
        want = np.sqrt(x)
    _assert_bitwise("sqrt", x, _device(gpu, 1, x), want)


def test_reciprocal_is_ieee(gpu):
    rs = np.random.RandomState(2)

    def signed(b):
        return _from_bits(b | (rs.randint(0, 2, b.size, dtype=np.uint64) << np.uint64(63)))

    binades = signed(rs.randint(0, 0x7FF0000000000000, 5_000_000, dtype=np.uint64))
    subnormal = signed(rs.randint(1, 1 << 52, 1_500_000, dtype=np.uint64))
    huge = signed(rs.randint(0x7FD0000000000000, 0x7FF0000000000000, 2_000_000, dtype=np.uint64))  # |x| >= 2^1022
    unit = rs.uniform(1.0, 2.0, 1_000_000) * rs.choice([-1.0, 1.0], 1_000_000)
    x = np.r_[binades, subnormal, huge, unit, 0.0, -0.0, np.inf, -np.inf, np.nan, _near(_powers_of_two())]
    with np.errstate(divide="ignore", over="ignore"):
        want = 1.0 / x
    _assert_bitwise("reciprocal", x, _device(gpu, 2, x), want)


def _ulps_from_exact_cube(v, g):
    """|g - v^3| in units of the last place of v^3 rounded (inf: whether v^3 rounds to g = +-inf)"""
    exact = Fraction(v) ** 3
    big = Fraction(2**1024 - 2**970)  # DBL_MAX + half an ulp: from here on v^3 rounds to +-inf
    if abs(exact) >= big:
        return 0.0 if g == math.copysign(math.inf, v) else math.inf
    if math.isinf(g):
        return math.inf
    return float(abs(Fraction(g) - exact) / Fraction(float(np.spacing(abs(float(exact))))))


def test_nielsen_cube(gpu):
    """lm_cube: the device's form (lm_cube_fma, pl_refine.h) bit for bit; within one ulp of the exact cube; glibc's
    pow(x, 3) - what the reference calls - for >= 99.9 % of the arguments"""
    rs = np.random.RandomState(12)
    regular = np.r_[rs.uniform(-1.0, 1.0, 1_000_000), rs.uniform(-4.0, 4.0, 500_000),
                    10.0 ** rs.uniform(-8, 3, 500_000) * rs.choice([-1.0, 1.0], 500_000)]
    # the branches of lm_cube_fma, and 1e+-100 where they used to be
    branch = _near([2.0**-360, 2.0**-330, 1e-100, 1e100, 2.0**330, 2.0**342])
    wide = _log_uniform(rs, 1e-120, 1e110, 20_000)
    x = np.r_[regular, branch, wide, 0.0, -0.0, 1.0, -1.0, 0.5, 1 / 3, np.inf, -np.inf, np.nan]
    got = _device(gpu, 0, x)
    _assert_bitwise("cube: device vs host lm_cube_fma", x, got, HM.lm_cube(x))
    ex = np.r_[rs.choice(regular, 200_000, replace=False), branch, wide]
    ulps = np.array([_ulps_from_exact_cube(v, g) for v, g in zip(ex.tolist(), _device(gpu, 0, ex).tolist())])
    print(f"cube: at most {ulps.max():.3f} ulp from the exact cube on {ex.size} arguments")
    assert (ulps <= 1.0).all(), f"cube: {int((ulps > 1).sum())} of {ex.size} more than one ulp off; first {float(ex[ulps > 1][0]).hex()}"
    fin = np.isfinite(x)
    pw = HM.glibc("pow3", x[fin])
    rate = float((_bits(got[fin]) == _bits(pw)).mean())
    print(f"cube: equal to glibc pow(x, 3) for {100.0 * rate:.4f} % of {int(fin.sum())} arguments")
    assert rate >= 0.999, rate


# ---- fp16 conversions of the matrix-core pre-filters (fn 9 .. 11: bit patterns as integer-valued doubles) ----------------
def _half_is_nan(b):
    b = np.asarray(b).astype(np.uint32)
    return ((b & 0x7C00) == 0x7C00) & ((b & 0x3FF) != 0)


def _assert_half_bits(name, v, got, want):
    got, want = np.asarray(got).astype(np.int64), np.asarray(want).astype(np.int64)
    bad = (got != want) & ~(_half_is_nan(got) & _half_is_nan(want))
    msg = _report(name, v.astype(np.float64), bad, got, want)
    assert not msg, msg


def _half_arguments():
    """float32: for every finite fp16 h >= 0 the midpoint to its successor and one float32 ulp on either side, the overflow
    edge, 2^-25, float32 subnormals, +-0, inf - both signs - and NaN; then 4e6 values randn 10^U(-9, 5)"""
    h = np.arange(0, 0x7C00, dtype=np.uint16)
    val = h.view(np.float16).astype(np.float32)
    succ = (h + np.uint16(1)).view(np.float16).astype(np.float32)
    mid = ((val + succ) / np.float32(2))[:-1]  # (exact: 12 significant bits)
    mids = np.r_[mid, np.nextafter(mid, np.float32(0)), np.nextafter(mid, np.float32(np.inf))]
    rs = np.random.RandomState(16)
    sub32 = np.r_[np.float32(1.4e-45), np.nextafter(np.float32(2.0**-126), np.float32(0)),
                  rs.randint(1, 1 << 23, 10_000).astype(np.uint32).view(np.float32)]
    f32 = np.float32
    edge = np.r_[f32(65504), f32(65520), np.nextafter(f32(65520), f32(0)), f32(2.0**-25), f32(0), f32(np.inf)]
    pos = np.r_[mids, val, sub32, edge].astype(np.float32)
    rnd = (rs.standard_normal(4_000_000) * 10.0 ** rs.uniform(-9, 5, 4_000_000)).astype(np.float32)
    return np.r_[pos, -pos, rnd, f32(np.nan)].astype(np.float32)


def test_half_round_to_nearest_is_ieee(gpu):
    v = _half_arguments()
    with np.errstate(over="ignore"):
        want = v.astype(np.float16).view(np.uint16)
    _assert_half_bits("pf_half_rn", v, _device(gpu, 9, v.astype(np.float64)), want)


def test_half_to_float_is_ieee(gpu):
    h = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)
    with np.errstate(invalid="ignore"):
        want = h.view(np.float16).astype(np.float32).astype(np.float64)
    _assert_bitwise("pf_half_to_float", h.astype(np.float64), _device(gpu, 10, h.astype(np.float64)), want)


def test_half_round_up_is_the_smallest_half_not_below(gpu):
    v = _half_arguments()
    v = v[v >= 0]
    with np.errstate(over="ignore"):
        h = v.astype(np.float16)
        below = h.astype(np.float32) < v
        want = np.where(below, np.nextafter(h, np.float16(np.inf)), h).view(np.uint16)
    _assert_half_bits("pf_half_up", v, _device(gpu, 11, v.astype(np.float64)), want)
