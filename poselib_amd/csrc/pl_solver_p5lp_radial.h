// poselib_amd — register-resident radial P5LP for one lane (one RANSAC iteration per lane): absolute pose of a camera with
// unknown radial distortion from five 2D-3D correspondences (Kukelova et al., ICCV 2013, as used by the reference).
//
// A point on the ray from the centre through the pixel x constrains the first two rows of [R | t] linearly:
// x_x (r_2 X + t_y) - x_y (r_1 X + t_x) = 0.  Five such rows leave a three-dimensional null space of the eight unknowns
// (PoseLib/solvers/p5lp_radial.cc:48-62: the last three columns of Q of a Householder QR of the 8x5 coefficient matrix),
// the orthonormality of the two rows gives two quadrics in its two free coefficients, their resultant is a quartic
// (p5lp_radial.cc:64-120), and every real root is completed to a pose (p5lp_radial.cc:122-173).
//
// Everything follows the reference operation for operation - Householder vectors, tau == 0 branches and the row order of
// every inner product as the reference build's QR forms them, the association of the resultant's polynomial coefficients
// (p5lp_radial.cc:65-110, BSD-3 source: the arithmetic ORDER is what bit-parity requires, so that block is a transliteration
// by design), the quartic of PoseLib/misc/univariate.cc:184-235 - so that set, ORDER and bits of the solutions equal the CPU
// path's.  Only the last three columns of Q are formed: every column of Q depends on the reflectors alone and is updated
// independently of the others.
#pragma once
#include "pl_math.h"
#include "pl_solver_p3p.h"

namespace pl {

// univariate.cc:48-61.  Returns false when there is no real root.
PL_HD bool quadratic_real_roots(double a, double b, double c, double &r0, double &r1) {
    const double b2m4ac = b * b - 4 * a * c;
    if (b2m4ac < 0)
        return false;
    const double sq = sqrt(b2m4ac);
    r0 = (b > 0) ? (2 * c) / (-b - sq) : (2 * c) / (-b + sq);
    r1 = c / (a * r0);
    return true;
}

// univariate.cc:184-235: real roots of x^4 + b x^3 + c x^2 + d x + e through one real root of the resolvent cubic
// (cubic_one_real_root, pl_solver_p3p.h), one Newton step per root.  roots[] is written with constant indices only.
PL_HD int quartic_real_roots(double b, double c, double d, double e, double *roots /*[4]*/) {
    const double p = c - 3.0 * b * b / 8.0;
    const double q = b * b * b / 8.0 - 0.5 * b * c + d;
    const double r = (-3.0 * b * b * b * b + 256.0 * e - 64.0 * b * d + 16.0 * b * b * c) / 256.0;

    const double bb = 2.0 * p;
    const double cc = p * p - 4.0 * r;
    const double dd = -q * q;

    double u2;
    cubic_one_real_root(bb, cc, dd, u2);
    if (u2 < 0)
        return 0;
    const double u = sqrt(u2);
    const double s = -u;
    const double t = (p + u * u + q / u) / 2.0;
    const double v = (p + u * u - q / u) / 2.0;

    // the two quadratic factors; the second pair follows the first in the list (univariate.cc:210-222)
    double pa0 = 0, pa1 = 0, pb0 = 0, pb1 = 0;
    const double disc_a = u * u - 4.0 * v;
    const bool have_a = disc_a > 0;
    if (have_a) {
        pa0 = (-u - (u < 0 ? -1.0 : 1.0) * sqrt(disc_a)) / 2.0;
        pa1 = v / pa0;
    }
    const double disc_b = s * s - 4.0 * t;
    const bool have_b = disc_b > 0;
    if (have_b) {
        pb0 = (-s - (s < 0 ? -1.0 : 1.0) * sqrt(disc_b)) / 2.0;
        pb1 = t / pb0;
    }
    roots[0] = have_a ? pa0 : pb0;
    roots[1] = have_a ? pa1 : pb1;
    roots[2] = pb0;
    roots[3] = pb1;
    const int sols = (have_a ? 2 : 0) + (have_b ? 2 : 0);
    PL_UNROLL
    for (int i = 0; i < 4; ++i)
        if (i < sols) {
            const double x = roots[i] - b / 4.0;
            const double x2 = x * x;
            const double x3 = x * x2;
            const double dx = -(x2 * x2 + b * x3 + c * x2 + d * x + e) / (4.0 * x3 + 3.0 * b * x2 + 2.0 * c * x + d);
            roots[i] = x + dx;
        }
    return sols;
}

// The last three columns of Q = householderQr().householderQ() of the 8x5 matrix A (A[r][c], destroyed), N[r][j] = Q(r, 5 + j).
PL_HD void householder_null3_8x5(double (&A)[8][5], double (&N)[8][3]) {
    double tau[5];
    PL_UNROLL
    for (int k = 0; k < 5; ++k) {
        double tail_sq = 0.0;
        PL_UNROLL
        for (int r = k + 1; r < 8; ++r)
            tail_sq += A[r][k] * A[r][k];
        const double c0 = A[k][k];
        double beta;
        if (tail_sq <= 2.2250738585072014e-308) { // numeric_limits<double>::min()
            tau[k] = 0.0;
            beta = c0;
            PL_UNROLL
            for (int r = k + 1; r < 8; ++r)
                A[r][k] = 0.0;
        } else {
            beta = sqrt(c0 * c0 + tail_sq);
            if (c0 >= 0.0)
                beta = -beta;
            PL_UNROLL
            for (int r = k + 1; r < 8; ++r)
                A[r][k] = A[r][k] / (c0 - beta);
            tau[k] = (beta - c0) / beta;
        }
        A[k][k] = beta;
        const double tk = tau[k];
        if (tk != 0.0) {
            PL_UNROLL
            for (int c = k + 1; c < 5; ++c) {
                double t = 0.0;
                PL_UNROLL
                for (int r = k + 1; r < 8; ++r)
                    t += A[r][k] * A[r][c];
                t += A[k][c];
                A[k][c] -= tk * t;
                PL_UNROLL
                for (int r = k + 1; r < 8; ++r)
                    A[r][c] -= tk * A[r][k] * t;
            }
        }
    }
    PL_UNROLL
    for (int r = 0; r < 8; ++r)
        PL_UNROLL
        for (int j = 0; j < 3; ++j)
            N[r][j] = (r == 5 + j) ? 1.0 : 0.0;
    PL_UNROLL
    for (int k = 4; k >= 0; --k) {
        const double tk = tau[k];
        if (tk != 0.0) {
            PL_UNROLL
            for (int j = 0; j < 3; ++j) {
                double t = 0.0;
                PL_UNROLL
                for (int r = k + 1; r < 8; ++r)
                    t += A[r][k] * N[r][j];
                t += N[k][j];
                N[k][j] -= tk * t;
                PL_UNROLL
                for (int r = k + 1; r < 8; ++r)
                    N[r][j] -= tk * A[r][k] * t;
            }
        }
    }
}

// x: the five 2-D points (the estimator hands in unit vectors, absolute_pose.cc:357), X: the 3-D points.  Every solution goes to
// emit(m, R, t) in the reference's order; returns their number (<= 4): roots whose quadratic has no real solution are skipped
// (p5lp_radial.cc:137-138), so it is the size of the reference's output, not its return value.  t.z = 0 / scale.
template <typename Emit> PL_HD int p5lp_radial_emit(const double (&x)[5][2], const double (&X)[5][3], Emit &&emit) {
    double A[8][5];
    PL_UNROLL
    for (int i = 0; i < 5; ++i) {
        A[0][i] = -x[i][1] * X[i][0];
        A[1][i] = -x[i][1] * X[i][1];
        A[2][i] = -x[i][1] * X[i][2];
        A[3][i] = -x[i][1];
        A[4][i] = x[i][0] * X[i][0];
        A[5][i] = x[i][0] * X[i][1];
        A[6][i] = x[i][0] * X[i][2];
        A[7][i] = x[i][0];
    }
    double N[8][3];
    householder_null3_8x5(A, N);

    // coefficients of the two quadrics and of their resultant (p5lp_radial.cc:65-110)
    const double h1 = N[0][1] * N[4][1] + N[1][1] * N[5][1] + N[2][1] * N[6][1];
    const double b1 = N[0][1] * N[4][2] + N[0][2] * N[4][1] + N[1][1] * N[5][2] + N[1][2] * N[5][1] + N[2][1] * N[6][2] +
        N[2][2] * N[6][1];
    const double b2 = N[0][0] * N[4][1] + N[0][1] * N[4][0] + N[1][0] * N[5][1] + N[1][1] * N[5][0] + N[2][0] * N[6][1] +
        N[2][1] * N[6][0];
    const double g1 = N[0][2] * N[4][2] + N[1][2] * N[5][2] + N[2][2] * N[6][2];
    const double g2 = N[0][0] * N[4][2] + N[0][2] * N[4][0] + N[1][0] * N[5][2] + N[1][2] * N[5][0] + N[2][0] * N[6][2] +
        N[2][2] * N[6][0];
    const double g3 = N[0][0] * N[4][0] + N[1][0] * N[5][0] + N[2][0] * N[6][0];
    const double d1 = N[0][1] * N[0][1] + N[1][1] * N[1][1] + N[2][1] * N[2][1] - N[4][1] * N[4][1] - N[5][1] * N[5][1] -
        N[6][1] * N[6][1];
    const double e1 = 2 * N[0][1] * N[0][2] + 2 * N[1][1] * N[1][2] + 2 * N[2][1] * N[2][2] - 2 * N[4][1] * N[4][2] -
        2 * N[5][1] * N[5][2] - 2 * N[6][1] * N[6][2];
    const double e2 = 2 * N[0][0] * N[0][1] + 2 * N[1][0] * N[1][1] + 2 * N[2][0] * N[2][1] - 2 * N[4][0] * N[4][1] -
        2 * N[5][0] * N[5][1] - 2 * N[6][0] * N[6][1];
    const double f1 = N[0][2] * N[0][2] + N[1][2] * N[1][2] + N[2][2] * N[2][2] - N[4][2] * N[4][2] - N[5][2] * N[5][2] -
        N[6][2] * N[6][2];
    const double f2 = 2 * N[0][0] * N[0][2] + 2 * N[1][0] * N[1][2] + 2 * N[2][0] * N[2][2] - 2 * N[4][0] * N[4][2] -
        2 * N[5][0] * N[5][2] - 2 * N[6][0] * N[6][2];
    const double f3 = N[0][0] * N[0][0] + N[1][0] * N[1][0] + N[2][0] * N[2][0] - N[4][0] * N[4][0] - N[5][0] * N[5][0] -
        N[6][0] * N[6][0];
    double k4 = h1 * h1 * f3 * f3 - h1 * b2 * e2 * f3 - 2 * h1 * g3 * d1 * f3 +
        h1 * g3 * e2 * e2 + b2 * b2 * d1 * f3 - b2 * g3 * d1 * e2 +
        g3 * g3 * d1 * d1;
    double k3 = h1 * g2 * e2 * e2 + 2 * g2 * g3 * d1 * d1 + b2 * b2 * d1 * f2 +
        2 * h1 * h1 * f2 * f3 - h1 * b1 * e2 * f3 - h1 * b2 * e1 * f3 -
        h1 * b2 * e2 * f2 - 2 * h1 * g2 * d1 * f3 - 2 * h1 * g3 * d1 * f2 +
        2 * h1 * g3 * e1 * e2 + 2 * b1 * b2 * d1 * f3 - b1 * g3 * d1 * e2 -
        b2 * g2 * d1 * e2 - b2 * g3 * d1 * e1;
    double k2 = h1 * h1 * f2 * f2 + g2 * g2 * d1 * d1 + h1 * g1 * e2 * e2 +
        h1 * g3 * e1 * e1 + 2 * g1 * g3 * d1 * d1 + b2 * b2 * d1 * f1 +
        b1 * b1 * d1 * f3 + 2 * h1 * h1 * f1 * f3 - h1 * b1 * e1 * f3 -
        h1 * b1 * e2 * f2 - h1 * b2 * e1 * f2 - h1 * b2 * e2 * f1 -
        2 * h1 * g1 * d1 * f3 - 2 * h1 * g2 * d1 * f2 +
        2 * h1 * g2 * e1 * e2 - 2 * h1 * g3 * d1 * f1 +
        2 * b1 * b2 * d1 * f2 - b1 * g2 * d1 * e2 - b1 * g3 * d1 * e1 -
        b2 * g1 * d1 * e2 - b2 * g2 * d1 * e1;
    double k1 = h1 * g2 * e1 * e1 + 2 * g1 * g2 * d1 * d1 + b1 * b1 * d1 * f2 +
        2 * h1 * h1 * f1 * f2 - h1 * b1 * e1 * f2 - h1 * b1 * e2 * f1 -
        h1 * b2 * e1 * f1 - 2 * h1 * g1 * d1 * f2 + 2 * h1 * g1 * e1 * e2 -
        2 * h1 * g2 * d1 * f1 + 2 * b1 * b2 * d1 * f1 - b1 * g1 * d1 * e2 -
        b1 * g2 * d1 * e1 - b2 * g1 * d1 * e1;
    double k0 = h1 * h1 * f1 * f1 - h1 * b1 * e1 * f1 - 2 * h1 * g1 * d1 * f1 +
        h1 * g1 * e1 * e1 + b1 * b1 * d1 * f1 - b1 * g1 * d1 * e1 +
        g1 * g1 * d1 * d1;

    k4 = 1.0 / k4;
    k3 *= k4;
    k2 *= k4;
    k1 *= k4;
    k0 *= k4;

    double roots[4];
    const int n_roots = quartic_real_roots(k3, k2, k1, k0, roots);

    int n = 0;
    PL_UNROLL
    for (int i = 0; i < 4; ++i)
        if (i < n_roots) {
            const double a = roots[i];
            const double c1a = h1;
            const double c1b = b1 + b2 * a;
            const double c1c = g1 + g2 * a + g3 * a * a;
            const double c2a = d1;
            const double c2b = e1 + e2 * a;
            const double c2c = f1 + f2 * a + f3 * a * a;
            double bb0, bb1;
            if (quadratic_real_roots(c1a, c1b, c1c, bb0, bb1)) {
                const double res1 = c2a * bb0 * bb0 + c2b * bb0 + c2c;
                // points in a plane (all X_z = 0): one solution only, the second one is NaN (p5lp_radial.cc:144-149)
                const double res2 = (bb1 != bb1) ? 1.7976931348623157e308 : c2a * bb1 * bb1 + c2b * bb1 + c2c;
                const double b = (fabs(res1) > fabs(res2)) ? bb1 : bb0;
                double p[8];
                PL_UNROLL
                for (int r = 0; r < 8; ++r)
                    p[r] = N[r][0] * a + N[r][1] * b + N[r][2];
                const double scale = sqrt(0.0 + p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
                Mat3 R;
                R.m[0] = p[0] / scale, R.m[1] = p[1] / scale, R.m[2] = p[2] / scale;
                R.m[3] = p[4] / scale, R.m[4] = p[5] / scale, R.m[5] = p[6] / scale;
                Vec3 t = v3(p[3] / scale, p[7] / scale, 0.0 / scale);
                set_row(R, 2, cross(row(R, 0), row(R, 1)));
                // the sign that puts the first point on the pixel's side of the centre
                const double s0 = R.m[0] * X[0][0] + R.m[1] * X[0][1] + R.m[2] * X[0][2] + t.x;
                const double s1 = R.m[3] * X[0][0] + R.m[4] * X[0][1] + R.m[5] * X[0][2] + t.y;
                if (0.0 + s0 * x[0][0] + s1 * x[0][1] < 0) {
                    PL_UNROLL
                    for (int e = 0; e < 6; ++e)
                        R.m[e] = -R.m[e];
                    t = -t;
                }
                emit(n, R, t);
                ++n;
            }
        }
    return n;
}

// a 2-D vector over its length: Eigen's normalized() (a division by the norm, not a multiplication by its reciprocal)
PL_HD void normalized2(double x, double y, double &ox, double &oy) {
    const double n = sqrt(0.0 + x * x + y * y);
    ox = x / n;
    oy = y / n;
}

} // namespace pl
