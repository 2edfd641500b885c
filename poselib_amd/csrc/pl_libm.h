// poselib_amd — libm functions whose LAST BIT matters for parity, restated so that the device rounds like the
// reference's host library instead of like ocml.
//
// The reference calls std::cbrt / std::acos / std::cos in the cubic solvers of P3P and the 7-point solver
// (PoseLib/misc/univariate.cc:82, 86, 107-124).  Those come from the C library of the machine the reference runs on -
// glibc 2.35 (libm.so.6, sysdeps/ieee754/dbl-64) in this image - a third-party dependency that is not vendored in
// /root/reference.  glibc's results are faithfully rounded, not correctly rounded, so "the same function from another
// vendor" (ocml) differs in the last bit for a sizeable share of the arguments; the models of a minimal sample then
// differ in their last bits, which decides ties between models of the same sample drawn twice (small N).
//
//   pl_cbrt : glibc's algorithm (s_cbrt.c, unchanged since glibc 2.0): frexp, a degree-6 polynomial for the
//             mantissa's cube root, one Halley step, 2^(e mod 3 / 3) from a table, ldexp.  Plain IEEE operations in
//             a fixed order, no FMA (the x86-64 build of s_cbrt.c has no FMA variant) => bit-identical to the host's
//             cbrt for every argument; tests/test_libm_vs_glibc.py checks 2e7 arguments against the host libm.
//   pl_cos  : glibc's IBM Accurate Mathematical Library routine (s_sin.c: __cos, do_cos, do_sin, reduce_sincos): the
//             argument is split at multiples of 1/128, sin / cos of the grid point come from a double-double table
//             (regenerated from first principles by scripts/gen_libm_tables.py), the remainder from short polynomials.
//   pl_acos : e_asin.c __ieee754_acos: a polynomial below 1/8, piecewise expansions of asin around the midpoints of
//             intervals of width 2^-8 up to 31/32 (asincos.tbl), and 2 asin(sqrt((1 - |x|) / 2)) with an inline
//             double-double square root above.
//             Both are restated as the operation sequence of the variant glibc selects on hosts with FMA
//             (__cos_fma / __acos_fma: the same source compiled with -mfma, i.e. with GCC's contractions) - every
//             fused multiply-add below is one in that binary, everything else is a separately rounded operation.
//             tests/test_libm_vs_glibc.py checks both bit for bit against the host's libm (2e7 arguments each).
//             A host without FMA would run glibc's sse2 variant, whose results differ in the last bit for a small
//             share of the arguments - the oracle then differs from this header exactly as it differs from itself
//             on another machine.
//   pl_atan2, pl_tan : e_atan2.c __ieee754_atan2 and s_tan.c __tan, FMA variants, for the fisheye camera models
//             (misc/camera_models.cc:1049, 1190, ...); tables uatan.tbl / utan.tbl.  tests/test_libm_trig_vs_glibc.py checks
//             both bit for bit against the host's libm (2e7 arguments each), tests/test_gpu_device_math2.py on the device.
//   pl_log1p : s_log1p.c, for the Cauchy losses' cost (robust/robust_loss.h); no FMA variant, see below.
#pragma once
#include "pl_defs.h"

#define PL_TABLE static constexpr
#include "pl_libm_tables.h"
#undef PL_TABLE

namespace pl {

PL_HD double pl_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }
PL_HD uint32_t pl_hi(double v) {
    uint64_t b;
    __builtin_memcpy(&b, &v, 8);
    return (uint32_t)(b >> 32);
}
PL_HD uint32_t pl_lo(double v) {
    uint64_t b;
    __builtin_memcpy(&b, &v, 8);
    return (uint32_t)b;
}

// ---- cos (s_sin.c) ---------------------------------------------------------------------------------------------------
namespace libm_detail {
constexpr double kSn3 = -1.66666666666664880952546298448555E-01, kSn5 = 8.33333214285722277379541354343671E-03;
constexpr double kCs2 = 4.99999999999999999999950396842453E-01, kCs4 = -4.16666666666664434524222570944589E-02,
                 kCs6 = 1.38888874007937613028114285595617E-03;
constexpr double kS1 = -0x1.5555555555555p-3, kS2 = 0x1.1111111110ECEp-7, kS3 = -0x1.A01A019DB08B8p-13,
                 kS4 = 0x1.71DE27B9A7ED9p-19, kS5 = -0x1.ADDFFC2FCDF59p-26;
constexpr double kBig = 0x1.8p45;                                        // 1.5 * 2^45: rounds to multiples of 2^-7
constexpr double kHp0 = 0x1.921FB54442D18p0, kHp1 = 0x1.1A62633145C07p-54; // pi / 2 in two parts

// FMA = true: the operation sequence of glibc's -mfma variants (__sin_fma / __cos_fma: every mad below is ONE fused operation in
// that binary); FMA = false: the same source without contractions (the sse2 build - what `sincos` is on x86-64: it has no FMA variant)
template <bool FMA> PL_HD double mad(double a, double b, double c) {
    if constexpr (FMA)
        return pl_fma(a, b, c);
    else
        return a * b + c;
}
template <bool FMA = true> PL_HD double do_cos(double x, double dx) {
    if (x < 0)
        dx = -dx;
    const double u = kBig + fabs(x);
    const int k = (int)pl_lo(u);
    x = fabs(x) - (u - kBig) + dx;
    const double xx = x * x;
    const double s = mad<FMA>(x * xx, mad<FMA>(xx, kSn5, kSn3), x);
    const double c = xx * mad<FMA>(xx, mad<FMA>(xx, kCs6, kCs4), kCs2);
    const double sn = kSinCosTab[k][0], ssn = kSinCosTab[k][1], cs = kSinCosTab[k][2], ccs = kSinCosTab[k][3];
    const double cor = mad<FMA>(-s, sn, mad<FMA>(-c, cs, mad<FMA>(-s, ssn, ccs)));
    return cs + cor;
}
template <bool FMA = true> PL_HD double do_sin(double x, double dx) {
    const double xold = x;
    if (fabs(x) < 0.126) { // TAYLOR_SIN
        const double xx = x * x;
        const double p = mad<FMA>(xx, mad<FMA>(xx, mad<FMA>(xx, mad<FMA>(xx, kS5, kS4), kS3), kS2), kS1);
        const double t = mad<FMA>(xx, mad<FMA>(p, x, -(0.5 * dx)), dx);
        return x + t;
    }
    if (x <= 0)
        dx = -dx;
    const double u = kBig + fabs(x);
    const int k = (int)pl_lo(u);
    x = fabs(x) - (u - kBig);
    const double xx = x * x;
    const double s = x + mad<FMA>(x * xx, mad<FMA>(xx, kSn5, kSn3), dx);
    const double c = mad<FMA>(dx, x, xx * mad<FMA>(xx, mad<FMA>(xx, kCs6, kCs4), kCs2));
    const double sn = kSinCosTab[k][0], ssn = kSinCosTab[k][1], cs = kSinCosTab[k][2], ccs = kSinCosTab[k][3];
    const double cor = mad<FMA>(s, cs, mad<FMA>(-c, sn, mad<FMA>(s, ccs, ssn)));
    return copysign(sn + cor, xold);
}
} // namespace libm_detail

// Domain of pl_cos / pl_sin / pl_sincos - a contract, checked on the device by tests/test_gpu_device_math.py: glibc's bits
// for |x| < 105414350 (cos, sincos) and |x| < 2.426265 (sin).  Beyond it glibc switches to another reduction that is not
// restated here: the device library's cos / sin answer instead (finite for finite x, not glibc's last bit).  The kernels stay
// inside: the cubic solvers' cos arguments lie in [-4.2, 1.1], quat_exp's sincos argument is half an LM rotation step.
PL_HD double pl_cos(double x) {
    using namespace libm_detail;
    const uint32_t k = pl_hi(x) & 0x7fffffffu;
    if (k < 0x3e400000u) // |x| < 2^-27
        return 1.0;
    if (k < 0x3feb6000u) // |x| < 0.855469
        return do_cos(x, 0.0);
    if (k < 0x400368fdu) { // |x| < 2.426265
        const double y = kHp0 - fabs(x);
        const double a = y + kHp1;
        const double da = (y - a) + kHp1;
        return do_sin(a, da);
    }
    if (k < 0x419921FBu) { // reduce_sincos: x - n pi / 2 with pi / 2 in four parts
        constexpr double hpinv = 0x1.45F306DC9C883p-1, toint = 0x1.8p52;
        constexpr double mp1 = 0x1.921FB58000000p0, mp2 = -0x1.DDE973C000000p-27, pp3 = -0x1.CB3B398000000p-55,
                         pp4 = -0x1.d747f23e32ed7p-83;
        const double t = pl_fma(x, hpinv, toint);
        const double xn = t - toint;
        const double y = pl_fma(-xn, mp2, pl_fma(-xn, mp1, x));
        int n = (int)(pl_lo(t) & 3u);
        double t1 = xn * pp3;
        const double t2 = y - t1;
        double db = (y - t2) - t1;
        t1 = xn * pp4;
        const double b = t2 - t1;
        db += (t2 - b) - t1;
        n = n + 1;
        const double r = (n & 1) ? do_cos(b, db) : do_sin(b, db);
        return (n & 2) ? -r : r;
    }
    return cos(x); // outside the domain (not reached by the solvers)
}

// s_sin.c __sin on the domain |x| < 2.426265 (above)
PL_HD double pl_sin(double x) {
    using namespace libm_detail;
    const uint32_t k = pl_hi(x) & 0x7fffffffu;
    if (k < 0x3e500000u) // |x| < 2^-26
        return x;
    if (k < 0x3feb6000u)
        return do_sin(x, 0.0);
    if (k < 0x400368fdu) {
        const double t = kHp0 - fabs(x);
        return copysign(do_cos(t, kHp1), x);
    }
    return sin(x); // outside the domain
}

// sin and cos of the SAME argument: s_sincos.c __sincos, the sse2 build (libm exports one `sincos`, without an FMA variant).
// quat_exp (misc/quaternion.h:73-96) calls std::cos and std::sin on theta / 2; GCC merges the two calls into one sincos()
// at -O1 and above, so the reference's Release build - and the oracle - step their quaternions with THESE roundings, which
// differ from sin() / cos() of the same machine in the last bit for 0.1 % (sin) and 0.03 % (cos) of the arguments below 0.86
// (measured on 2*10^7 arguments; found by scripts/soak_intrinsics.py as a one-ulp difference of an LM step).
// tests/test_libm_vs_glibc.py checks it bit for bit against the host's sincos().
PL_HD void pl_sincos(double x, double &sn, double &cs) {
    using namespace libm_detail;
    const uint32_t k = pl_hi(x) & 0x7fffffffu;
    if (k < 0x400368fdu) {
        if (k < 0x3e400000u) { // |x| < 2^-27
            sn = x;
            cs = 1.0;
            return;
        }
        if (k < 0x3feb6000u) { // |x| < 0.855469
            sn = do_sin<false>(x, 0.0);
            cs = do_cos<false>(x, 0.0);
            return;
        }
        const double y = kHp0 - fabs(x); // |x| < 2.426265
        const double a = y + kHp1;
        const double da = (y - a) + kHp1;
        sn = copysign(do_cos<false>(a, da), x);
        cs = do_sin<false>(a, da);
        return;
    }
    if (k < 0x419921FBu) { // reduce_sincos + do_sincos(n), do_sincos(n + 1)
        constexpr double hpinv = 0x1.45F306DC9C883p-1, toint = 0x1.8p52;
        constexpr double mp1 = 0x1.921FB58000000p0, mp2 = -0x1.DDE973C000000p-27, pp3 = -0x1.CB3B398000000p-55,
                         pp4 = -0x1.d747f23e32ed7p-83;
        const double t = x * hpinv + toint;
        const double xn = t - toint;
        const double y = (x - xn * mp1) - xn * mp2;
        const int n = (int)(pl_lo(t) & 3u);
        double t1 = xn * pp3;
        const double t2 = y - t1;
        double db = (y - t2) - t1;
        t1 = xn * pp4;
        const double b = t2 - t1;
        db += (t2 - b) - t1;
        auto pick = [&](int m) {
            const double r = (m & 1) ? do_cos<false>(b, db) : do_sin<false>(b, db);
            return (m & 2) ? -r : r;
        };
        sn = pick(n);
        cs = pick(n + 1);
        return;
    }
    sn = sin(x); // outside the domain (rotation increments of an LM step never get here)
    cs = cos(x);
}

// ---- acos (e_asin.c __ieee754_acos, FMA variant) -----------------------------------------------------------------------
PL_HD double pl_acos(double x) {
    using namespace libm_detail;
    // (uasncs.h: the odd polynomial of asin near 0, also used for asin(sqrt(z)) near |x| = 1)
    constexpr double f1 = 0x1.55555555554f9p-3, f2 = 0x1.333333336127dp-4, f3 = 0x1.6db6dae42c0e4p-5,
                     f4 = 0x1.f1c7e04f4ad99p-6, f5 = 0x1.6e442c822d419p-6, f6 = 0x1.292d80f453c72p-6;
    const uint32_t hi = pl_hi(x);
    const int32_t m = (int32_t)hi;
    const uint32_t k = hi & 0x7fffffffu;
    if (k < 0x3c880000u) // |x| < 2^-55
        return kHp0;
    if (k < 0x3fc00000u) { // |x| < 1/8
        const double x2 = x * x;
        const double p = pl_fma(x2, pl_fma(x2, pl_fma(x2, pl_fma(x2, pl_fma(x2, f6, f5), f4), f3), f2), f1);
        const double r = kHp0 - x;
        const double e = ((kHp0 - r) - x) + kHp1;
        return r + pl_fma(-p, x * x2, e);
    }
    if (k < 0x3fef0000u) { // 1/8 <= |x| < 31/32: expansion of asin around the midpoint of the argument's interval
        int n, nc; // row start, number of coefficients
        if (k < 0x3fd00000u)
            n = 11 * (int)((k >> 15) & 0x1fu), nc = 6;
        else if (k < 0x3fe00000u)
            n = 11 * (int)((k >> 14) & 0x3fu) + 352, nc = 6;
        else if (k < 0x3fe80000u)
            n = 12 * (int)((k >> 13) & 0x7fu) + 1056, nc = 7;
        else if (k < 0x3fed8000u)
            n = 13 * (int)((k >> 13) & 0x7fu) + 992, nc = 8;
        else if (k < 0x3fee8000u)
            n = 14 * (int)((k >> 13) & 0x7fu) + 884, nc = 9;
        else
            n = 15 * (int)((k >> 13) & 0x7fu) + 768, nc = 10;
        const double *T = kAsinRows + n;
        const double ax = (m > 0) ? x : -x;
        const double xx = ax - T[0];
        double p = T[nc];
        for (int j = nc - 1; j >= 2; --j)
            p = pl_fma(xx, p, T[j]);
        p = pl_fma(xx * xx, p, T[nc + 1]); // + asin(x0) low part
        const double t = pl_fma(xx, T[1], p);
        const double y = T[nc + 2]; // asin(x0) high part
        if (m > 0)
            return (kHp1 - t) + (kHp0 - y);
        return (t + kHp1) + (y + kHp0);
    }
    if (k < 0x3ff00000u) { // 31/32 <= |x| < 1: 2 asin(sqrt(z)), z = (1 - |x|) / 2, sqrt(z) as y + cc
        constexpr double rt0 = 0x1.fffffffecc1ddp-1, rt1 = 0x1.fffffff757304p-2, rt2 = 0x1.800496769c91ap-2,
                         rt3 = 0x1.4006318d1dab9p-2, t27 = 134217728.0; // (uasncs.h: inverse square root refinement)
        const double z = ((m > 0) ? (1.0 - x) : (x + 1.0)) * 0.5;
        const uint32_t zh = pl_hi(z);
        const int e = (int)(zh >> 21); // (sign bit clear)
        uint64_t pw = (uint64_t)(1023 + (511 - e)) << 52; // powtwo[511 - e] = 2^(511 - e)
        double two;
        __builtin_memcpy(&two, &pw, 8);
        double t = kInvRoot[(zh >> 14) & 0x7fu] * two;
        const double r = pl_fma(-(t * t), z, 1.0);
        t = pl_fma(r, pl_fma(r, pl_fma(r, rt3, rt2), rt1), rt0) * t;
        const double c = z * t;
        const double h = pl_fma(-(t * 0.5), c, 1.5);
        const double w = pl_fma(c, t27, c);
        const double y = pl_fma(-t27, c, w);
        const double den = pl_fma(h, c, y);
        const double cc = pl_fma(-y, y, z) / den;
        const double p = pl_fma(z, pl_fma(z, pl_fma(z, pl_fma(z, pl_fma(z, f6, f5), f4), f3), f2), f1) * z;
        const double cor = p * (y + cc);
        if (m > 0) {
            const double s = (cc + cor) + y;
            return s + s;
        }
        const double s = ((kHp1 - cc) - cor) + (kHp0 - y);
        return s + s;
    }
    if (k == 0x3ff00000u && pl_lo(x) == 0u) // |x| = 1
        return (m > 0) ? 0.0 : 0x1.921FB54442D18p1;
    if (k > 0x7ff00000u || (k == 0x7ff00000u && pl_lo(x) != 0u))
        return x + x; // NaN
    return (x - x) / (x - x); // |x| > 1
}

// ---- atan2 (e_atan2.c __ieee754_atan2, FMA variant) ----------------------------------------------------------------------
// The fisheye projections call std::atan2(rho, z) (misc/camera_models.cc:1049, 1072, ...).  glibc 2.35's routine has one stage
// (the multi-precision fall-backs left in 2.34): u = min(|x|, |y|) / max(|x|, |y|) with its rounding error du from an exact product,
// then the odd polynomial below 1/16 or the expansion around the table point of u's interval of width 2^-8 (uatan.tbl), and the
// result assembled per quadrant with pi / 2 or pi in two parts.  Restated as the operation sequence of __ieee754_atan2_fma.
//
// Domain - a contract, checked bit for bit on the host (tests/test_libm_trig_vs_glibc.py) and on the device
// (tests/test_gpu_device_math2.py): glibc's bits for every finite x and every finite y != 0 (the cameras call it with
// y = rho > 1e-8).  y = 0, infinities and NaN go to the plain atan2.  The thresholds, named as in e_atan2.c:
namespace libm_detail {
constexpr int32_t ATAN2_EP = 59768832;           // exponent difference (high words) from which y / x is "infinite": 57 << 20
constexpr double ATAN2_TWO500 = 0x1p500, ATAN2_TWOM500 = 0x1p-500; // |x| or |y| beyond: both are scaled
constexpr double ATAN2_INV16 = 0.0625;           // u below: polynomial, from it on: table
constexpr double kAd3 = -0x1.5555555555555p-2, kAd5 = 0x1.99999999997fdp-3, kAd7 = -0x1.24924923f7603p-3,
                 kAd9 = 0x1.c71c6e5129a3bp-4, kAd11 = -0x1.7458022b13c25p-4, kAd13 = 0x1.375f08b31cbcep-4; // (uatan.tbl d3 .. d13)
constexpr double kOpi = 0x1.921FB54442D18p1, kOpi1 = 0x1.1A62633145C07p-53; // pi in two parts (kHp0, kHp1: pi / 2)
PL_HD double atan_poly13(double v) {
    return pl_fma(pl_fma(pl_fma(pl_fma(pl_fma(kAd13, v, kAd11), v, kAd9), v, kAd7), v, kAd5), v, kAd3);
}
PL_HD int atan_row(double u) { // i = (TWO52 + TWO8 * u) - TWO52 as an int, minus 16: the nearest multiple of 1 / 256 (ties to even)
    return (int)(pl_fma(u, 256.0, 0x1p52) - 0x1p52) - 16;
}
} // namespace libm_detail

PL_HD double pl_atan2(double y, double x) {
    using namespace libm_detail;
    const uint32_t ux = pl_hi(x), uy = pl_hi(y);
    if ((ux & 0x7ff00000u) == 0x7ff00000u || (uy & 0x7ff00000u) == 0x7ff00000u || y == 0.0)
        return atan2(y, x); // outside the domain
    if (x == 0.0)
        return (uy & 0x80000000u) ? -kHp0 : kHp0;
    double ax = (x < 0) ? -x : x, ay = (y < 0) ? -y : y;
    const int32_t de = (int32_t)(uy & 0x7ff00000u) - (int32_t)(ux & 0x7ff00000u);
    if (de >= ATAN2_EP)
        return (y > 0) ? kHp0 : -kHp0;
    if (de <= -ATAN2_EP) {
        if (x > 0)
            return copysign(ay / ax, y);
        return (y > 0) ? kOpi : -kOpi;
    }
    if (ax < ATAN2_TWOM500 || ay < ATAN2_TWOM500) {
        ax *= ATAN2_TWO500;
        ay *= ATAN2_TWO500;
    }
    if (ax > ATAN2_TWO500 || ay > ATAN2_TWO500) {
        ax *= ATAN2_TWOM500;
        ay *= ATAN2_TWOM500;
    }
    // u + du = min / max: the quotient, and the quotient of the exact remainder
    const bool y_small = ay < ax;
    const double num = y_small ? ay : ax, den = y_small ? ax : ay;
    const double u = num / den;
    const double pv = den * u;
    const double pvv = pl_fma(den, u, -pv);
    const double du = ((num - pv) - pvv) / den;
    double z;
    if (x > 0 && y_small) { // (i) atan(ay / ax)
        if (u < ATAN2_INV16) {
            const double v = u * u;
            z = u + pl_fma(u * v, atan_poly13(v), du);
        } else {
            const double *c = kAtanRows[atan_row(u)];
            const double t3 = u - c[0];
            const double v = t3 + du;
            const double dv = (fabs(t3) > fabs(du)) ? ((t3 - v) + du) : ((du - v) + t3);
            const double p = (v * v) * pl_fma(pl_fma(pl_fma(c[6], v, c[5]), v, c[4]), v, c[3]);
            z = pl_fma(v, c[2], pl_fma(dv, c[2], p)) + c[1];
        }
        return copysign(z, y);
    }
    // (ii) x > 0: pi / 2 - atan(ax / ay)   (iii) x < 0, |x| < |y|: pi / 2 + atan(ax / ay)   (iv) x < 0: pi - atan(ay / ax)
    const bool plus = !(x > 0) && !(ay <= ax);
    const bool whole = !(x > 0) && (ay <= ax);
    const double P = whole ? kOpi : kHp0, P1 = whole ? kOpi1 : kHp1;
    if (u < ATAN2_INV16) {
        const double v = u * u;
        const double zz = (u * v) * atan_poly13(v);
        if (plus) {
            const double t2 = P + u;
            const double cor = (P > fabs(u)) ? ((P - t2) + u) : ((u - t2) + P);
            z = (((cor + P1) + du) + zz) + t2;
        } else {
            const double t2 = P - u;
            const double cor = (P > fabs(u)) ? ((P - t2) - u) : (P - (u + t2));
            z = (((cor + P1) - du) - zz) + t2;
        }
    } else {
        const double *c = kAtanRows[atan_row(u)];
        const double v = (u - c[0]) + du;
        const double p = pl_fma(pl_fma(pl_fma(pl_fma(c[6], v, c[5]), v, c[4]), v, c[3]), v, c[2]);
        if (plus)
            z = (P + c[1]) + pl_fma(v, p, P1);
        else
            z = (P - c[1]) + pl_fma(-v, p, P1);
    }
    return copysign(z, y);
}

// pl_atan2 out of line: the LM kernels (k_lm<0> sits at 255 VGPRs) reach it only for a fisheye camera; inlined, its registers cost
// k_lm, k_lm_ordered, k_lm2 and k_lm_cam scratch on EVERY camera (profiles/fisheye_registers.md)
PL_HD_CALL double pl_atan2_call(double y, double x) { return pl_atan2(y, x); }

// ---- tan (s_tan.c __tan, FMA variant) ---------------------------------------------------------------------------------------
// The fisheye un-projections call 1.0 / std::tan(theta) (misc/camera_models.cc:1190).  Polynomial up to 0.0608, up to 0.787
// tan(x0 + z) = f + z' (g + f) / (g - z') around the table point x0 (utan.tbl: f = tan x0, g = cot x0), beyond that the argument is
// reduced by multiples of pi / 2 in three parts and the same two forms give tan or -cot.
//
// Domain - the same kind of contract as pl_cos: glibc's bits for |x| <= TAN_DOMAIN_MAX = 25 (s_tan.c's g4; the Newton result of
// the un-projection lies in [0, pi) whenever it converges).  Beyond it glibc reduces with more parts of pi / 2, which is not
// restated: the plain tan answers (finite for finite x, not glibc's last bit); infinities and NaN give NaN as in glibc.
// The thresholds, named as in utan.h:
namespace libm_detail {
constexpr double TAN_G1 = 0x1.b096cp-27;         // |x| up to 1.259e-8: x
constexpr double TAN_G2 = 0x1.f212dp-5;          // up to 0.0608: polynomial (also of the reduced argument)
constexpr double TAN_G3 = 0x1.92f1ap-1;          // up to 0.787: table
constexpr double TAN_DOMAIN_MAX = 25.0;          // g4: up to here the three-part reduction
constexpr double kTd3 = 0x1.5555555555555p-2, kTd5 = 0x1.11111111107c6p-3, kTd7 = 0x1.ba1ba1cdb8745p-5,
                 kTd9 = 0x1.664ed49cfc666p-6, kTd11 = 0x1.2385a3cf2e4eap-7; // (utan.h d3 .. d11)
constexpr double kTe0 = 0x1.5555555554dbdp-2, kTe1 = 0x1.11112e0a6b45fp-3;
constexpr double kTmp3 = -0x1.cb3b399d747f2p-55; // third part of pi / 2 (mp1, mp2 as in pl_cos)
PL_HD double tan_poly11(double v) { return pl_fma(pl_fma(pl_fma(pl_fma(kTd11, v, kTd9), v, kTd7), v, kTd5), v, kTd3); }
// table form: w in (TAN_G2, TAN_G3], dw its low part; cot = false: tan(w + dw), cot = true: cot(w + dw)
PL_HD double tan_table(double w, double dw, bool cot) {
    const int i = (int)pl_fma(256.0, w, -15.5);
    const double z = (w - kTanRows[i][0]) + dw;
    const double z2 = z * z;
    const double pz = pl_fma(z * z2, pl_fma(z2, kTe1, kTe0), z);
    const double fi = kTanRows[i][1], gi = kTanRows[i][2];
    const double num = (fi + gi) * pz;
    return cot ? gi - num / (pz + fi) : num / (gi - pz) + fi;
}
} // namespace libm_detail

PL_HD double pl_tan(double x) {
    using namespace libm_detail;
    if ((pl_hi(x) & 0x7ff00000u) == 0x7ff00000u)
        return x - x;
    const double w = (x < 0.0) ? -x : x;
    if (w <= TAN_G1)
        return x;
    if (w <= TAN_G2) {
        const double x2 = x * x;
        return pl_fma(x * x2, tan_poly11(x2), x);
    }
    if (w <= TAN_G3) {
        const double s = (x < 0.0) ? -1.0 : 1.0;
        return tan_table(w, 0.0, false) * s; // (w - x0 + 0.0 = w - x0: it is never -0)
    }
    if (!(w <= TAN_DOMAIN_MAX))
        return tan(x); // outside the domain
    constexpr double hpinv = 0x1.45F306DC9C883p-1, toint = 0x1.8p52;
    constexpr double mp1 = 0x1.921FB58000000p0, mp2 = -0x1.DDE973C000000p-27;
    const double t = pl_fma(x, hpinv, toint);
    const double xn = t - toint;
    const uint32_t n = pl_lo(t) & 1u;
    const double t1 = pl_fma(-xn, mp2, pl_fma(-xn, mp1, x));
    const double a = pl_fma(-xn, kTmp3, t1);
    const double da = pl_fma(-xn, kTmp3, t1 - a);
    const bool neg = a < 0.0;
    const double ya = neg ? -a : a, yya = neg ? -da : da, sy = neg ? -1.0 : 1.0;
    if (ya <= TAN_G2) {
        const double a2 = a * a;
        const double t2 = pl_fma(a * a2, tan_poly11(a2), da);
        const double y = a + t2;
        if (!n)
            return y;
        // -cot: 1 / (b + db) in double-double arithmetic (EADD, DIV2)
        const double b = y;
        const double db = (fabs(a) > fabs(t2)) ? ((a - b) + t2) : ((t2 - b) + a);
        const double c = 1.0 / b;
        const double p = c * b;
        const double pp = pl_fma(c, b, -p);
        const double cc = pl_fma(-db, c, ((1.0 - p) - pp) + 0.0) / b;
        const double z = c + cc;
        const double zz = (c - z) + cc;
        return -(zz + z);
    }
    return n ? tan_table(ya, yya, true) * -sy : tan_table(ya, yya, false) * sy;
}

PL_HD double pl_cbrt(double x) {
    // frexp of |x|: xm in [0.5, 1), |x| = xm 2^xe  (glibc's frexp sets xe = 0 for 0, inf, NaN)
    uint64_t bits;
    const double ax = fabs(x);
    __builtin_memcpy(&bits, &ax, 8);
    int ex = (int)(bits >> 52);
    if (ex == 0x7ff || ax == 0.0)
        return x + x; // s_cbrt.c: "if (xe == 0 && fpclassify (x) <= FP_ZERO) return x + x"
    int xe;
    if (ex == 0) { // subnormal: normalise first (frexp multiplies by 2^54)
        const double sc = ax * 18014398509481984.0;
        __builtin_memcpy(&bits, &sc, 8);
        ex = (int)(bits >> 52);
        xe = ex - 1022 - 54;
    } else {
        xe = ex - 1022;
    }
    bits = (bits & 0x000fffffffffffffull) | 0x3fe0000000000000ull;
    double xm;
    __builtin_memcpy(&xm, &bits, 8);

    const double u = (0.354895765043919860 +
                      ((1.50819193781584896 -
                        ((2.11499494167371287 -
                          ((2.44693122563534430 -
                            ((1.83469277483613086 - (0.784932344976639262 - 0.145263899385486377 * xm) * xm) * xm)) *
                           xm)) *
                         xm)) *
                       xm));
    const double t2 = u * u * u;
    // factor[2 + xe % 3] with C's truncating remainder: {1 / 2^(2/3), 1 / 2^(1/3), 1, 2^(1/3), 2^(2/3)}
    const int rem = xe % 3;
    const double cbrt2 = 1.2599210498948731648, sqr_cbrt2 = 1.5874010519681994748;
    const double f = rem == -2 ? 1.0 / sqr_cbrt2 : rem == -1 ? 1.0 / cbrt2 : rem == 0 ? 1.0 : rem == 1 ? cbrt2 : sqr_cbrt2;
    const double ym = u * (t2 + 2.0 * xm) / (2.0 * t2 + xm) * f;
    // ldexp(+-ym, xe / 3): ym in [0.39, 1.6), the result of a finite argument never leaves the normal range
    const int q = xe / 3;
    double r = x > 0.0 ? ym : -ym;
    uint64_t rb;
    __builtin_memcpy(&rb, &r, 8);
    rb += (uint64_t)(int64_t)q << 52;
    __builtin_memcpy(&r, &rb, 8);
    return r;
}

// ---- log1p (s_log1p.c) -----------------------------------------------------------------------------------------------
// The Cauchy losses' cost term (robust_loss.h: sq * log1p(r2 / sq)).  glibc's routine is fdlibm's: 1 + x = 2^k (1 + f) with
// sqrt(2) / 2 < 1 + f < sqrt(2), the rounding error of 1 + x carried as c, log(1 + f) = f - f^2 / 2 + s (f^2 / 2 + R(s^2)) with
// s = f / (2 + f) and a degree-14 polynomial R - in glibc evaluated in four independent pairs (R1 .. R4 below), which is what
// makes its last bit differ from fdlibm's Horner form on one argument in 10^4.  Plain IEEE operations in a fixed order, no FMA
// (glibc 2.35 has no FMA variant of s_log1p.c) => bit-identical to the host's log1p; tests/test_lm_cam_cases.py checks 2e7
// arguments against the host libm.  ocml's log1p differs from it in the last bit often enough that a Nielsen update after a
// mediocre step (pl_refine.h lm_cube) took another lambda than the reference: two of the 104 bundle adjustments of tests/lm_cam_cases.py under a Cauchy loss and the Nielsen update
// ended in other last bits than the serial host model.
PL_HD double pl_log1p(double x) {
    constexpr double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10, two54 = 1.80143985094819840000e+16;
    constexpr double Lp1 = 6.666666666666735130e-01, Lp2 = 3.999999999940941908e-01, Lp3 = 2.857142874366239149e-01,
                     Lp4 = 2.222219843214978396e-01, Lp5 = 1.818357216161805012e-01, Lp6 = 1.531383769920937332e-01,
                     Lp7 = 1.479819860511658591e-01;
    auto with_hi = [](double v, int32_t h) {
        uint64_t b;
        __builtin_memcpy(&b, &v, 8);
        b = (b & 0xffffffffull) | ((uint64_t)(uint32_t)h << 32);
        __builtin_memcpy(&v, &b, 8);
        return v;
    };
    const int32_t hx = (int32_t)pl_hi(x), ax = hx & 0x7fffffff;
    int32_t k = 1, hu = 0;
    double f = 0.0, c = 0.0, u;
    if (hx < 0x3FDA827A) { // x < 0.41422
        if (ax >= 0x3ff00000)  // x <= -1: -inf at -1, NaN below
            return (x == -1.0) ? -two54 / 0.0 : (x - x) / (x - x);
        if (ax < 0x3e200000) // |x| < 2^-29
            return (two54 + x > 0.0 && ax < 0x3c900000) ? x : x - x * x * 0.5;
        if (hx > 0 || hx <= (int32_t)0xbfd2bec3) { // -0.2929 < x < 0.41422
            k = 0;
            f = x;
            hu = 1;
        }
    }
    if (hx >= 0x7ff00000)
        return x + x;
    if (k != 0) {
        if (hx < 0x43400000) {
            u = 1.0 + x;
            hu = (int32_t)pl_hi(u);
            k = (hu >> 20) - 1023;
            c = (k > 0) ? 1.0 - (u - x) : x - (u - 1.0); // the correction term
            c /= u;
        } else {
            u = x;
            hu = (int32_t)pl_hi(u);
            k = (hu >> 20) - 1023;
            c = 0.0;
        }
        hu &= 0x000fffff;
        if (hu < 0x6a09e) {
            u = with_hi(u, hu | 0x3ff00000); // normalise u
        } else {
            k += 1;
            u = with_hi(u, hu | 0x3fe00000); // normalise u / 2
            hu = (0x00100000 - hu) >> 2;
        }
        f = u - 1.0;
    }
    const double hfsq = 0.5 * f * f;
    if (hu == 0) { // |f| < 2^-20
        if (f == 0.0) {
            if (k == 0)
                return 0.0;
            c += k * ln2_lo;
            return k * ln2_hi + c;
        }
        const double R = hfsq * (1.0 - 0.66666666666666666 * f);
        return (k == 0) ? f - R : k * ln2_hi - ((R - (k * ln2_lo + c)) - f);
    }
    const double s = f / (2.0 + f);
    const double z = s * s;
    const double R1 = z * Lp1, z2 = z * z;
    const double R2 = Lp2 + z * Lp3, z4 = z2 * z2;
    const double R3 = Lp4 + z * Lp5, z6 = z4 * z2;
    const double R4 = Lp6 + z * Lp7;
    const double R = R1 + z2 * R2 + z4 * R3 + z6 * R4;
    return (k == 0) ? f - (hfsq - s * (hfsq + R)) : k * ln2_hi - ((hfsq - (s * (hfsq + R) + (k * ln2_lo + c))) - f);
}

} // namespace pl
