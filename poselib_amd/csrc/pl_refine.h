// poselib_amd — Levenberg-Marquardt building blocks for local optimisation (LO) and the final
// polish.  The per-correspondence residual / Jacobian functions and the LM control logic are
// PL_HD: the device kernel (kernels.hip, one workgroup per refinement task, reductions through
// DPP + LDS) and the host-side unit test build share this file.
//
// Reference semantics followed (citations relative to /root/reference/PoseLib):
//   robust/optim/lm_impl.h:56-140            LM driver (Nielsen / fixed-factor lambda, stop rules)
//   robust/optim/jacobian_accumulator.h      normal equations; NOTE the single residual_count that
//                                            both passes overwrite (:62-64,78-82,166) — reproduced.
//   robust/robust_loss.h:59-157              losses
//   robust/optim/absolute.h:40-171           reprojection refiner (no intrinsics refined)
//   robust/optim/relative.h:39-166           Sampson refiner on (R, t) with a tangent basis for t
//   robust/optim/homography.h:46-178         symmetric transfer error, 8 parameters
//   robust/optim/fundamental.h:41-121 + optim_utils.h:57-82   Sampson on the Bartoli-Sturm factorisation
//   misc/camera_models.cc:668-755,919-1032,2704-2726  projections with Jacobians (NULL, SIMPLE_PINHOLE,
//                                            PINHOLE, OPENCV)
//   misc/camera_models.cc:579-611,764-913    SIMPLE_RADIAL and RADIAL: radial polynomial, Newton inverse
//   misc/camera_models.cc:613-662,1044-1201,1517-1652,1664-1790   OPENCV_FISHEYE, SIMPLE_RADIAL_FISHEYE, RADIAL_FISHEYE:
//                                            atan2 / tan through pl_libm.h, the Newton inverse of the polynomial in theta
#pragma once
#include "pl_math.h"
#include "pl_score.h"

namespace pl {

enum LossType : int { LOSS_TRIVIAL = 0, LOSS_TRUNCATED, LOSS_HUBER, LOSS_CAUCHY, LOSS_TRUNCATED_CAUCHY, LOSS_TRUNCATED_LE_ZACH };
enum CameraId : int {
    CAM_NULL = -1,
    CAM_SIMPLE_PINHOLE = 0,
    CAM_PINHOLE = 1,
    CAM_SIMPLE_RADIAL = 2,
    CAM_RADIAL = 3,
    CAM_OPENCV = 4,
    CAM_OPENCV_FISHEYE = 5,
    CAM_SIMPLE_RADIAL_FISHEYE = 8,
    CAM_RADIAL_FISHEYE = 9
};
// SIMPLE_RADIAL (f cx cy k1) and RADIAL (f cx cy k1 k2): one focal length, a polynomial in the squared radius
PL_HD bool camera_is_radial(int model_id) { return model_id == CAM_SIMPLE_RADIAL || model_id == CAM_RADIAL; }
// models whose un-projection is iterative: max(|x|, |y|) of the un-projected points cannot be bounded from the pixels on the host
// OPENCV_FISHEYE (fx fy cx cy k1 k2 k3 k4), SIMPLE_RADIAL_FISHEYE (f cx cy k) and RADIAL_FISHEYE (f cx cy k1 k2): the radius in
// the image is a polynomial in the angle theta to the optical axis
PL_HD bool camera_is_fisheye(int model_id) {
    return model_id == CAM_OPENCV_FISHEYE || model_id == CAM_SIMPLE_RADIAL_FISHEYE || model_id == CAM_RADIAL_FISHEYE;
}
// parameter layout: fx fy cx cy ... (two focal lengths) or f cx cy ... (one)
PL_HD bool camera_has_two_focals(int model_id) { return model_id == CAM_PINHOLE || model_id == CAM_OPENCV || model_id == CAM_OPENCV_FISHEYE; }
PL_HD bool camera_is_nonlinear(int model_id) { return model_id == CAM_OPENCV || camera_is_radial(model_id) || camera_is_fisheye(model_id); }

struct LMOptions {
    uint32_t max_iterations;
    int32_t loss_type, lambda_update, damping;
    double loss_scale, gradient_tol, step_tol, relative_cost_tol, initial_lambda, min_lambda, max_lambda, lambda_factor;
};

// ------------------------------------------------------------------------------------ losses
struct Loss {
    int type;
    double thr, sq, inv_sq, max_loss, mu;
};
PL_HD Loss make_loss(int type, double scale) {
    Loss l;
    l.type = type;
    l.thr = scale;
    l.sq = scale * scale;
    l.inv_sq = 1.0 / l.sq;
    l.max_loss = l.sq * pl_log1p(1.0);
    l.mu = 0.5;
    return l;
}
PL_HD double loss_value(const Loss &l, double r2) {
    switch (l.type) {
    case LOSS_TRUNCATED:
    case LOSS_TRUNCATED_LE_ZACH:
        return fmin(r2, l.sq);
    case LOSS_HUBER: {
        const double r = sqrt(r2);
        return (r <= l.thr) ? r2 : l.thr * (2.0 * r - l.thr);
    }
    case LOSS_CAUCHY:
        return l.sq * pl_log1p(r2 * l.inv_sq);
    case LOSS_TRUNCATED_CAUCHY:
        return (r2 > l.sq) ? l.max_loss : l.sq * pl_log1p(r2 * l.inv_sq);
    default:
        return r2;
    }
}
PL_HD double loss_weight(const Loss &l, double r2) {
    const double dmin = 2.2250738585072014e-308;
    switch (l.type) {
    case LOSS_TRUNCATED:
        return (r2 < l.sq) ? 1.0 : 0.0;
    case LOSS_TRUNCATED_LE_ZACH: {
        const double rh = r2 / l.sq;
        const double zstar = fmin(rh, 1.0);
        if (rh < 1.0)
            return 0.5;
        const double m1 = rh - 1.0;
        const double rho = (2.0 * m1 + sqrt(4.0 * m1 * m1 * l.mu * l.mu + 2 * l.mu * m1)) / l.mu;
        const double a = (rh + l.mu * rho * zstar - 0.5 * rho) / (1 + l.mu * rho);
        const double zbar = fmax(0.0, fmin(a, 1.0));
        return (zstar - zbar) / rho;
    }
    case LOSS_HUBER: {
        const double r = sqrt(r2);
        return (r <= l.thr) ? 1.0 : l.thr / r;
    }
    case LOSS_CAUCHY:
        return fmax(dmin, 1.0 / (1.0 + r2 * l.inv_sq));
    case LOSS_TRUNCATED_CAUCHY:
        return (r2 > l.sq) ? 0.0 : fmax(dmin, 1.0 / (1.0 + r2 * l.inv_sq));
    default:
        return 1.0;
    }
}

// ------------------------------------------------------------------------------------ camera
struct CameraParams {
    int32_t model_id;
    int32_t num_params;
    double p[12];
};

PL_HD void opencv_distort(double k1, double k2, double p1, double p2, double u, double v, double &du, double &dv,
                          double *J /*2x2 row-major*/) {
    const double u2 = u * u, uv = u * v, v2 = v * v;
    const double r2 = u * u + v * v;
    J[0] = k2 * r2 * r2 + 6 * p2 * u + 2 * p1 * v + u * (2 * k1 * u + 4 * k2 * u * r2) + k1 * r2 + 1.0;
    J[1] = 2 * p1 * u + 2 * p2 * v + v * (2 * k1 * u + 4 * k2 * u * r2);
    J[2] = 2 * p1 * u + 2 * p2 * v + u * (2 * k1 * v + 4 * k2 * v * r2);
    J[3] = k2 * r2 * r2 + 2 * p2 * u + 6 * p1 * v + v * (2 * k1 * v + 4 * k2 * v * r2) + k1 * r2 + 1.0;
    const double alpha = 1.0 + k1 * r2 + k2 * r2 * r2;
    du = alpha * u + 2.0 * p1 * uv + p2 * (r2 + 2.0 * u2);
    dv = alpha * v + 2.0 * p2 * uv + p1 * (r2 + 2.0 * v2);
}

// camera_models.cc:579-611: the radius r with rd = (1 + k1 r^2 [+ k2 r^4]) r by Newton steps from r = rd (UNDIST_TOL 1e-10, at most
// UNDIST_MAX_ITER 100), every expression in the reference's order of operations
PL_HD double undistort_poly1(double k1, double rd) {
    double r = rd;
    for (int it = 0; it < 100; ++it) {
        const double r2 = r * r;
        const double f = k1 * r2 * r + r - rd;
        if (fabs(f) < 1e-10)
            break;
        const double fp = 3.0 * k1 * r2 + 1.0;
        r = r - f / fp;
    }
    return r;
}
PL_HD double undistort_poly2(double k1, double k2, double rd) {
    double r = rd;
    for (int it = 0; it < 100; ++it) {
        const double r2 = r * r;
        const double f = k2 * r2 * r2 * r + k1 * r2 * r + r - rd;
        if (fabs(f) < 1e-10)
            break;
        const double fp = 5.0 * k2 * r2 * r2 + 3.0 * k1 * r2 + 1.0;
        r = r - f / fp;
    }
    return r;
}

// camera_models.cc:613-662 undistort_theta_poly: theta with rd = theta (1 + sum_k params[k] theta^(2 (k - K0 + 1))), k = K0 ..
// num_params - 1 (the reference loops to params.size()), by Newton steps (UNDIST_TOL 1e-10, at most UNDIST_MAX_ITER 100) from 0,
// then - while the residual stays above the tolerance or theta comes out negative - from rd, rd / 2 and 3 rd / 2; what the last
// start leaves is returned, converged or not.  K0 is a template argument so that every parameter index is a constant.
template <int K0> PL_HD double undistort_theta_poly(const CameraParams &c, double rd) {
    double theta = 0.0;
    for (int start = 0; start < 4; ++start) {
        theta = (start == 0) ? 0.0 : (start == 1) ? rd : (start == 2) ? 0.5 * rd : 1.5 * rd;
        double f = 0.0;
        for (int it = 0; it < 100; ++it) {
            f = 1.0;
            double fp = 1.0;
            const double theta2 = theta * theta;
            double theta2k = theta2;
            double factor = 3.0;
            PL_UNROLL
            for (int k = K0; k < 12; ++k) {
                if (k >= c.num_params)
                    break;
                const double t = theta2k * c.p[k];
                f += t;
                fp += factor * t;
                theta2k *= theta2;
                factor += 2.0;
            }
            f *= theta;
            f -= rd;
            if (fabs(f) < 1e-10)
                break;
            theta = theta - f / fp;
        }
        if (!(fabs(f) > 1e-10 || theta < 0))
            break;
    }
    return theta;
}
// the fisheye models' parameters in one layout: k[j] multiplies theta^(2 j + 3); a coefficient the model lacks is +0.0, which
// leaves every sum below bit for bit what the reference's shorter expression gives (x + 0.0 = x, theta is finite)
struct FisheyeParams {
    double fx, fy, cx, cy, k[4];
};
PL_HD FisheyeParams fisheye_params(const CameraParams &c) {
    // (every parameter is read first and the layout chosen between VALUES: a choice between two elements of c.p would index the array at
    // run time, which costs the kernels that keep the camera in registers a scratch copy of it)
    const double p0 = c.p[0], p1 = c.p[1], p2 = c.p[2], p3 = c.p[3], p4 = c.p[4], p5 = c.p[5], p6 = c.p[6], p7 = c.p[7];
    const bool two = c.model_id == CAM_OPENCV_FISHEYE, k2 = c.model_id == CAM_RADIAL_FISHEYE;
    FisheyeParams f;
    f.fx = p0, f.fy = two ? p1 : p0, f.cx = two ? p2 : p1, f.cy = two ? p3 : p2;
    f.k[0] = two ? p4 : p3, f.k[1] = two ? p5 : (k2 ? p4 : 0.0), f.k[2] = two ? p6 : 0.0, f.k[3] = two ? p7 : 0.0;
    return f;
}
// camera_models.cc:1177-1201, 1628-1652, 1766-1790 followed by hnormalized (camera_models.h:98-102)
// ... the unit bearing itself (the models' 3-D unproject)
PL_HD Vec3 fisheye_unproject_bearing(const CameraParams &c, double px, double py) {
    const FisheyeParams f = fisheye_params(c);
    const double ux = (px - f.cx) / f.fx, uy = (py - f.cy) / f.fy;
    const double rd = sqrt(ux * ux + uy * uy);
    Vec3 b;
    if (rd > 1e-8) {
        const double theta = (c.model_id == CAM_OPENCV_FISHEYE) ? undistort_theta_poly<4>(c, rd) : undistort_theta_poly<3>(c, rd);
        b.x = ux / rd;
        b.y = uy / rd;
        if (fabs(theta - 1.57079632679489661923) > 1e-8)
            b.z = 1.0 / pl_tan(theta);
        else
            b.z = 0.0;
    } else {
        b.x = ux;
        b.y = uy;
        b.z = sqrt(1 - rd * rd);
    }
    return normalized(b);
}
PL_HD void fisheye_unproject(const CameraParams &c, double px, double py, double &ox, double &oy) {
    const Vec3 b = fisheye_unproject_bearing(c, px, py);
    ox = b.x / b.z;
    oy = b.y / b.z;
}
// camera_models.cc:1044-1157, 1517-1612, 1664-1764: project / project_with_jac of the three models.  J: d(xp)/dZ or nullptr; what
// the parameter columns need comes back in q = {inv_r, theta, theta2, rd} (theta < 0: the pinhole branch next to the axis).  JAC is a template argument: the residual pass carries none of the Jacobian's registers.
template <bool JAC> PL_HD void fisheye_project(const CameraParams &c, Vec3 Z, double &ox, double &oy, double *J, double *q) {
    const FisheyeParams f = fisheye_params(c);
    const double rho = sqrt(Z.x * Z.x + Z.y * Z.y);
    if (rho > 1e-8) {
        const double theta = pl_atan2_call(rho, Z.z);
        const double theta2 = theta * theta;
        const double theta4 = theta2 * theta2;
        const double theta6 = theta2 * theta4;
        const double theta8 = theta2 * theta6;
        const double rd = theta * (1.0 + theta2 * f.k[0] + theta4 * f.k[1] + theta6 * f.k[2] + theta8 * f.k[3]);
        const double inv_r = 1.0 / rho;
        if constexpr (JAC) {
            const double drho_dx = Z.x / rho;
            const double drho_dy = Z.y / rho;
            const double rho_z2 = rho * rho + Z.z * Z.z;
            const double dtheta_drho = Z.z / rho_z2;
            const double dtheta_dz = -rho / rho_z2;
            const double drd_dtheta = (1.0 + 3.0 * theta2 * f.k[0] + 5.0 * theta4 * f.k[1] + 7.0 * theta6 * f.k[2] + 9.0 * theta8 * f.k[3]);
            const double drd_dx = drd_dtheta * dtheta_drho * drho_dx;
            const double drd_dy = drd_dtheta * dtheta_drho * drho_dy;
            const double drd_dz = drd_dtheta * dtheta_dz;
            const double dinv_r_drho = -1.0 / (rho * rho);
            const double dinv_r_dx = dinv_r_drho * drho_dx;
            const double dinv_r_dy = dinv_r_drho * drho_dy;
            J[0] = f.fx * (inv_r * rd + Z.x * dinv_r_dx * rd + Z.x * inv_r * drd_dx);
            J[1] = f.fx * Z.x * (dinv_r_dy * rd + inv_r * drd_dy);
            J[2] = f.fx * Z.x * inv_r * drd_dz;
            J[3] = f.fy * Z.y * (dinv_r_dx * rd + inv_r * drd_dx);
            J[4] = f.fy * (inv_r * rd + Z.y * dinv_r_dy * rd + Z.y * inv_r * drd_dy);
            J[5] = f.fy * Z.y * inv_r * drd_dz;
            if (q)
                q[0] = inv_r, q[1] = theta, q[2] = theta2, q[3] = rd;
        }
        ox = f.fx * Z.x * inv_r * rd + f.cx;
        oy = f.fy * Z.y * inv_r * rd + f.cy;
    } else { // very close to the principal axis: the distortion is ignored
        ox = f.fx * Z.x + f.cx;
        oy = f.fy * Z.y + f.cy;
        if constexpr (JAC) {
            J[0] = f.fx, J[1] = 0.0, J[2] = 0.0;
            J[3] = 0.0, J[4] = f.fy, J[5] = 0.0;
            if (q)
                q[0] = 0.0, q[1] = -1.0, q[2] = 0.0, q[3] = 0.0;
        }
    }
}

// pixel -> bearing, the models' 3-D unproject: unit length, except the identity camera's (x, y, 1) (camera_models.cc:2724-2726)
PL_HD Vec3 camera_unproject_bearing(const CameraParams &c, double px, double py) {
    double u, v;
    switch (c.model_id) {
    case CAM_SIMPLE_PINHOLE:
        u = (px - c.p[1]) / c.p[0];
        v = (py - c.p[2]) / c.p[0];
        break;
    case CAM_PINHOLE:
        u = (px - c.p[2]) / c.p[0];
        v = (py - c.p[3]) / c.p[1];
        break;
    case CAM_OPENCV: {
        const double tx = (px - c.p[2]) / c.p[0], ty = (py - c.p[3]) / c.p[1];
        u = tx, v = ty;
        for (int it = 0; it < 100; ++it) { // camera_models.cc:972-990
            double du, dv, J[4];
            opencv_distort(c.p[4], c.p[5], c.p[6], c.p[7], u, v, du, dv, J);
            J[0] += 1e-8;
            J[3] += 1e-8;
            const double r0 = du - tx, r1 = dv - ty;
            if (sqrt(r0 * r0 + r1 * r1) < 1e-10)
                break;
            const double dt = J[0] * J[3] - J[2] * J[1];
            const double id = 1.0 / dt;
            const double s0 = (J[3] * id) * r0 + (-J[1] * id) * r1;
            const double s1 = (-J[2] * id) * r0 + (J[0] * id) * r1;
            u = u - s0;
            v = v - s1;
        }
        break;
    }
    case CAM_SIMPLE_RADIAL:
    case CAM_RADIAL: { // camera_models.cc:819-830, 895-907
        u = (px - c.p[1]) / c.p[0];
        v = (py - c.p[2]) / c.p[0];
        const double r0 = sqrt(u * u + v * v);
        if (fabs(r0) > 1e-8) {
            const double r = (c.model_id == CAM_RADIAL) ? undistort_poly2(c.p[3], c.p[4], r0) : undistort_poly1(c.p[3], r0);
            const double s = r / r0;
            u *= s;
            v *= s;
        }
        break;
    }
    case CAM_OPENCV_FISHEYE:
    case CAM_SIMPLE_RADIAL_FISHEYE:
    case CAM_RADIAL_FISHEYE:
        return fisheye_unproject_bearing(c, px, py);
    default: // CAM_NULL: bearing is (x, y, 1) un-normalised
        return v3(px, py, 1.0);
    }
    return normalized(v3(u, v, 1.0));
}
// pixel -> normalised image plane (camera_models.h:98-102: unit bearing first, then hnormalized)
PL_HD void camera_unproject(const CameraParams &c, double px, double py, double &ox, double &oy) {
    const Vec3 b = camera_unproject_bearing(c, px, py);
    ox = b.x / b.z;
    oy = b.y / b.z;
}

PL_HD void camera_project(const CameraParams &c, Vec3 Z, double &ox, double &oy) {
    switch (c.model_id) {
    case CAM_SIMPLE_PINHOLE:
        ox = c.p[0] * Z.x / Z.z + c.p[1];
        oy = c.p[0] * Z.y / Z.z + c.p[2];
        return;
    case CAM_PINHOLE:
        ox = c.p[0] * Z.x / Z.z + c.p[2];
        oy = c.p[1] * Z.y / Z.z + c.p[3];
        return;
    case CAM_OPENCV: {
        double du, dv, J[4];
        opencv_distort(c.p[4], c.p[5], c.p[6], c.p[7], Z.x / Z.z, Z.y / Z.z, du, dv, J);
        ox = c.p[0] * du + c.p[2];
        oy = c.p[1] * dv + c.p[3];
        return;
    }
    case CAM_SIMPLE_RADIAL: { // camera_models.cc:842-851: multiplies by 1 / z ...
        const double inv_z = 1.0 / Z.z;
        const double u = Z.x * inv_z, v = Z.y * inv_z;
        const double r2 = u * u + v * v;
        const double alpha = (1.0 + c.p[3] * r2);
        ox = c.p[0] * alpha * u + c.p[1];
        oy = c.p[0] * alpha * v + c.p[2];
        return;
    }
    case CAM_RADIAL: { // ... :767-773: divides by z (hnormalized), unlike its project_with_jac
        const double u = Z.x / Z.z, v = Z.y / Z.z;
        const double r2 = u * u + v * v;
        const double alpha = (1.0 + c.p[3] * r2 + c.p[4] * r2 * r2);
        ox = c.p[0] * alpha * u + c.p[1];
        oy = c.p[0] * alpha * v + c.p[2];
        return;
    }
    case CAM_OPENCV_FISHEYE:
    case CAM_SIMPLE_RADIAL_FISHEYE:
    case CAM_RADIAL_FISHEYE:
        fisheye_project<false>(c, Z, ox, oy, nullptr, nullptr);
        return;
    default:
        ox = Z.x / Z.z;
        oy = Z.y / Z.z;
    }
}
// camera_models.cc:774-818, 852-894: the radial models' project_with_jac up to jac = jac_d * [d(x/z, y/z)/dZ]; u, v, r2, alpha come
// back for the parameter columns (pl_refine_cam.h)
PL_HD void radial_project_jac(const CameraParams &c, Vec3 Z, double &ox, double &oy, double *J, double &u, double &v, double &r2,
                              double &alpha) {
    const double inv_z = 1.0 / Z.z;
    u = Z.x * inv_z, v = Z.y * inv_z;
    r2 = u * u + v * v;
    double Jd[4];
    if (c.model_id == CAM_RADIAL) {
        alpha = (1.0 + c.p[3] * r2 + c.p[4] * r2 * r2);
        const double alphap = (2.0 * c.p[3] + 4.0 * c.p[4] * r2);
        Jd[0] = (alphap * u * u + alpha) * c.p[0];
        Jd[1] = (alphap * u * v) * c.p[0];
        Jd[3] = (alphap * v * v + alpha) * c.p[0];
    } else {
        alpha = (1.0 + c.p[3] * r2);
        Jd[0] = (2.0 * c.p[3] * u * u + alpha) * c.p[0];
        Jd[1] = (2.0 * c.p[3] * u * v) * c.p[0];
        Jd[3] = (2.0 * c.p[3] * v * v + alpha) * c.p[0];
    }
    Jd[2] = Jd[1];
    const double P[6] = {inv_z, 0.0, -u * inv_z, 0.0, inv_z, -v * inv_z};
    PL_UNROLL
    for (int a = 0; a < 2; ++a)
        PL_UNROLL
        for (int b = 0; b < 3; ++b)
            J[3 * a + b] = Jd[2 * a] * P[b] + Jd[2 * a + 1] * P[3 + b];
    ox = c.p[0] * alpha * u + c.p[1];
    oy = c.p[0] * alpha * v + c.p[2];
}
// projection + d(xp)/dZ (2x3 row-major)
PL_HD void camera_project_jac(const CameraParams &c, Vec3 Z, double &ox, double &oy, double *J) {
    switch (c.model_id) {
    case CAM_SIMPLE_PINHOLE:
    case CAM_PINHOLE: {
        const bool simple = c.model_id == CAM_SIMPLE_PINHOLE;
        const double fx = c.p[0], fy = simple ? c.p[0] : c.p[1];
        const double cx = simple ? c.p[1] : c.p[2], cy = simple ? c.p[2] : c.p[3];
        const double zi = 1.0 / Z.z;
        const double px = fx * Z.x * zi, py = fy * Z.y * zi;
        J[0] = fx * zi, J[1] = 0.0, J[2] = -px * zi;
        J[3] = 0.0, J[4] = fy * zi, J[5] = -py * zi;
        ox = px + cx;
        oy = py + cy;
        return;
    }
    case CAM_OPENCV: {
        const double u = Z.x / Z.z, v = Z.y / Z.z;
        double du, dv, Jd[4];
        opencv_distort(c.p[4], c.p[5], c.p[6], c.p[7], u, v, du, dv, Jd);
        const double P[6] = {1.0 / Z.z, 0.0, -u / Z.z, 0.0, 1.0 / Z.z, -v / Z.z};
        PL_UNROLL
        for (int a = 0; a < 2; ++a)
            PL_UNROLL
            for (int b = 0; b < 3; ++b)
                J[3 * a + b] = Jd[2 * a] * P[b] + Jd[2 * a + 1] * P[3 + b];
        PL_UNROLL
        for (int b = 0; b < 3; ++b) {
            J[b] *= c.p[0];
            J[3 + b] *= c.p[1];
        }
        ox = c.p[0] * du + c.p[2];
        oy = c.p[1] * dv + c.p[3];
        return;
    }
    case CAM_SIMPLE_RADIAL:
    case CAM_RADIAL: {
        double u, v, r2, alpha;
        radial_project_jac(c, Z, ox, oy, J, u, v, r2, alpha);
        return;
    }
    case CAM_OPENCV_FISHEYE:
    case CAM_SIMPLE_RADIAL_FISHEYE:
    case CAM_RADIAL_FISHEYE:
        fisheye_project<true>(c, Z, ox, oy, J, nullptr);
        return;
    default: {
        ox = Z.x / Z.z;
        oy = Z.y / Z.z;
        const double zi = 1.0 / Z.z;
        J[0] = zi, J[1] = 0.0, J[2] = -ox * zi;
        J[3] = 0.0, J[4] = zi, J[5] = -oy * zi;
    }
    }
}

// Camera::unproject_with_jac (camera_models.cc:456-489): the bearing d of a pixel and M = d(d)/d(pixel), 3x2 row-major, as the
// pseudo-inverse of the projection's Jacobian at d:  J = project_with_jac(d) (2x3), B = J J^T, B^-1 = adj(B) / det, M = J^T B^-1.
// Every sum in the reference's order (k ascending).  False: det(B) is zero or not finite - M is then whatever the division gave.
PL_HD bool camera_unproject_with_jac(const CameraParams &c, double px, double py, Vec3 &d, double *M) {
    d = camera_unproject_bearing(c, px, py);
    double qx, qy, J[6];
    camera_project_jac(c, d, qx, qy, J);
    const double B00 = J[0] * J[0] + J[1] * J[1] + J[2] * J[2];
    const double B01 = J[0] * J[3] + J[1] * J[4] + J[2] * J[5];
    const double B10 = J[3] * J[0] + J[4] * J[1] + J[5] * J[2];
    const double B11 = J[3] * J[3] + J[4] * J[4] + J[5] * J[5];
    const double det = B00 * B11 - B01 * B10;
    const double I00 = B11 / det, I01 = -B01 / det, I10 = -B10 / det, I11 = B00 / det;
    PL_UNROLL
    for (int i = 0; i < 3; ++i) {
        M[2 * i] = J[i] * I00 + J[3 + i] * I10;
        M[2 * i + 1] = J[i] * I01 + J[3 + i] * I11;
    }
    return det != 0.0 && det - det == 0.0;
}

// ------------------------------------------------------------------------------------ accumulators
// Per-thread partial of the normal equations:  lower triangle of J^T J (row-major packed:
// (i,j), j<=i at i*(i+1)/2 + j) followed by J^T r.  Size K*(K+1)/2 + K.
template <int K> struct NormalSize {
    static constexpr int kTri = K * (K + 1) / 2;
    static constexpr int kTotal = kTri + K;
};

template <int K> PL_HD void accumulate2(double *acc, const Loss &loss, double r0, double r1, const double *J /*2xK*/,
                                        uint32_t &count) {
    const double w = 1.0 * loss_weight(loss, r0 * r0 + r1 * r1);
    if (w == 0)
        return;
    int o = 0;
    PL_UNROLL
    for (int i = 0; i < K; ++i)
        PL_UNROLL
        for (int j = 0; j <= i; ++j)
            acc[o++] += w * (J[i] * J[j] + J[K + i] * J[K + j]);
    const double wr0 = w * r0, wr1 = w * r1;
    PL_UNROLL
    for (int i = 0; i < K; ++i)
        acc[o + i] += J[i] * wr0 + J[K + i] * wr1;
    count++;
}
template <int K> PL_HD void accumulate1(double *acc, const Loss &loss, double r, const double *J /*K*/,
                                        uint32_t &count) {
    const double w = 1.0 * loss_weight(loss, r * r);
    if (w == 0)
        return;
    int o = 0;
    PL_UNROLL
    for (int i = 0; i < K; ++i)
        PL_UNROLL
        for (int j = 0; j <= i; ++j)
            acc[o++] += w * (J[i] * J[j]);
    const double wr = w * r;
    PL_UNROLL
    for (int i = 0; i < K; ++i)
        acc[o + i] += wr * J[i];
    count++;
}

// The same terms as accumulate2 / accumulate1, handed to `store(entry, value)` instead of added to an accumulator: k_lm's producers
// write them as a row of the term ring and the consumer adds row after row (the reference's `+=` per entry and correspondence,
// jacobian_accumulator.h:82-97).  `acc += v` with the value written here equals the reference's `acc += v` bit for bit; a
// correspondence with weight zero contributes nothing there (early return) and a row of zeros here (x + 0.0 = x).
template <int K, class Store> PL_HD void terms2(const Loss &loss, double r0, double r1, const double *J /*2xK*/, uint32_t &count, Store store) {
    const double w = 1.0 * loss_weight(loss, r0 * r0 + r1 * r1);
    if (w == 0) {
        PL_UNROLL
        for (int o = 0; o < NormalSize<K>::kTotal; ++o)
            store(o, 0.0);
        return;
    }
    int o = 0;
    PL_UNROLL
    for (int i = 0; i < K; ++i)
        PL_UNROLL
        for (int j = 0; j <= i; ++j)
            store(o++, w * (J[i] * J[j] + J[K + i] * J[K + j]));
    const double wr0 = w * r0, wr1 = w * r1;
    PL_UNROLL
    for (int i = 0; i < K; ++i)
        store(o + i, J[i] * wr0 + J[K + i] * wr1);
    count++;
}
template <int K, class Store> PL_HD void terms1(const Loss &loss, double r, const double *J /*K*/, uint32_t &count, Store store) {
    const double w = 1.0 * loss_weight(loss, r * r);
    if (w == 0) {
        PL_UNROLL
        for (int o = 0; o < NormalSize<K>::kTotal; ++o)
            store(o, 0.0);
        return;
    }
    int o = 0;
    PL_UNROLL
    for (int i = 0; i < K; ++i)
        PL_UNROLL
        for (int j = 0; j <= i; ++j)
            store(o++, w * (J[i] * J[j]));
    const double wr = w * r;
    PL_UNROLL
    for (int i = 0; i < K; ++i)
        store(o + i, wr * J[i]);
    count++;
}

// (2 rho - 1)^3 of the Nielsen update (lm_impl.h:124: std::pow(2.0 * rho - 1.0, 3)), see the note at lm_update
// The reference calls the host's libm here - glibc's pow, whose result for the exponent 3 is the correctly rounded cube
// for 99.9 % of the arguments (measured: 183 exceptions in 2*10^5; the device library's pow differs from it for 23 %).  The
// device therefore forms the (nearly) correctly rounded cube itself: x^2 = hi + lo and hi x = p + e exactly (FMA residuals), then
// one rounding of p + (e + lo x).  The value only matters for mediocre steps (factor = 1 - cube > 1/3, i.e. rho < 0.94).
// (the FMA form is a plain function so that the host test build can compare it with glibc's pow: tests/test_libm_vs_glibc.py)
PL_HD double lm_cube_two_product(double x) { // 2^-330 <= |x| <= 2^330: no residual overflows or underflows
    const double hi = x * x;
    const double lo = __builtin_fma(x, x, -hi);
    const double p = hi * x;
    const double e = __builtin_fma(hi, x, -p);
    return p + (e + lo * x); // (lo x and the inner sum round once each: NEARLY correctly rounded, see above)
}
PL_HD double lm_cube_fma(double x) {
    const double ax = fabs(x);
    if (ax >= 0x1p-330 && ax <= 0x1p330)
        return lm_cube_two_product(x);
    // beyond: the same form on x scaled by a power of two (exact), the cube scaled back - exact, or rounded once more into
    // the subnormal range (within one ulp, where x * x * x can be 1.5 ulp off)
    if (ax > 0x1p330 && ax < 0x1p342)
        return lm_cube_two_product(x * 0x1p-30) * 0x1p90;
    if (ax >= 0x1p-360 && ax < 0x1p-330)
        return lm_cube_two_product(x * 0x1p60) * 0x1p-180;
    return x * x * x; // 0, inf, NaN, cubes beyond the range (+-inf) or below half the smallest subnormal (+-0)
}
#if defined(PL_LM_CUBE_HOST_SWITCH) && !defined(__HIP_DEVICE_COMPILE__)
// (the test-only host build of tests/hostmath alone defines this: its LM then runs with the device's cube on request, so
// that it is a serial model of k_lm_ordered bit for bit, and keeps the cube's arguments; the product's host code always calls pow.
// One process-wide record without a lock: the test build runs its refinements one at a time, on one thread)
struct LMCubeHostSwitch {
    int device_form = 0;
    unsigned calls = 0;
    double args[256];
};
inline LMCubeHostSwitch &lm_cube_host_switch() {
    static LMCubeHostSwitch s;
    return s;
}
#endif
PL_HD double lm_cube(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return lm_cube_fma(x);
#elif defined(PL_LM_CUBE_HOST_SWITCH)
    LMCubeHostSwitch &s = lm_cube_host_switch();
    if (s.calls < 256)
        s.args[s.calls] = x;
    s.calls++;
    return s.device_form ? lm_cube_fma(x) : pow(x, 3);
#else
    return pow(x, 3);
#endif
}

// ------------------------------------------------------------------------------------ LM control
// Parameter block of a refinement task: 16 doubles.
//   absolute : [0..3] q, [4..6] t
//   relative : [0..3] q, [4..6] t, [7..9] tangent basis 0, [10..12] tangent basis 1
//   homography : [0..8] H row-major
//   fundamental: [0..3] qU, [4..7] qV, [8] sigma
constexpr int kParamDoubles = 16;

struct LMControl {
    LMOptions opt;
    Loss loss;
    double cost, initial_cost, lambda, nu, step_norm, grad_norm;
    uint32_t iterations, invalid_steps;
    uint32_t count; // the accumulator's single residual counter (see header comment)
    int32_t rejac;
    int32_t done;
    double sol[16]; // (up to 14: pose + 8 camera parameters, pl_refine_cam.h)
};

PL_HD double lm_scale(uint32_t count) { return 1.0 / fmax(1.0, (double)count); }

PL_HD void lm_begin(LMControl &c, const LMOptions &opt, double racc, uint32_t count) {
    c.opt = opt;
    c.count = count;
    c.cost = racc * lm_scale(count);
    c.initial_cost = c.cost;
    c.grad_norm = -1;
    c.step_norm = -1;
    c.invalid_steps = 0;
    c.lambda = opt.initial_lambda;
    c.nu = 2.0;
    c.rejac = 1;
    c.iterations = 0;
    c.done = (opt.max_iterations == 0) ? 1 : 0;
}

// After (optionally) a fresh Jacobian pass: gradient test, damped solve, step-size test.
// `normal` = reduced [tri | Jtr]; `jac_count` is the counter after the Jacobian pass (ignored when
// the Jacobian was not recomputed).  Sets c.done or leaves c.sol for the trial step.
template <int K> PL_HD void lm_solve(LMControl &c, const double *normal, bool fresh_jacobian, uint32_t jac_count) {
    constexpr int T = NormalSize<K>::kTri;
    if (fresh_jacobian) {
        c.count = jac_count;
        double s = 0;
        PL_UNROLL
        for (int i = 0; i < K; ++i)
            s += normal[T + i] * normal[T + i];
        c.grad_norm = lm_scale(c.count) * sqrt(s);
        if (c.grad_norm < c.opt.gradient_tol) {
            c.done = 1;
            return;
        }
    }
    const double sc = lm_scale(c.count);
    double A[K * K], b[K];
    PL_UNROLL
    for (int i = 0; i < K; ++i) {
        PL_UNROLL
        for (int j = 0; j <= i; ++j)
            A[i * K + j] = sc * normal[i * (i + 1) / 2 + j];
        b[i] = -(sc * normal[T + i]);
    }
    PL_UNROLL
    for (int i = 0; i < K; ++i)
        A[i * K + i] += (c.opt.damping == 1) ? fmax(A[i * K + i] * c.lambda, 1e-8) : c.lambda;
    // Cholesky with the operation order of Eigen's unblocked LLT (squared norm / dot product summed first, then
    // subtracted), forward solve by column-oriented updates, backward solve by row dot product then subtract
    PL_UNROLL
    for (int col = 0; col < K; ++col) {
        double d = A[col * K + col];
        if (col > 0) {
            double sq = A[col * K] * A[col * K];
            PL_UNROLL
            for (int m = 1; m < col; ++m)
                sq += A[col * K + m] * A[col * K + m];
            d -= sq;
        }
        if (d <= 0)
            break;
        d = sqrt(d);
        A[col * K + col] = d;
        PL_UNROLL
        for (int r = col + 1; r < K; ++r) {
            double s = A[r * K + col];
            if (col > 0) {
                double dot = A[r * K] * A[col * K];
                PL_UNROLL
                for (int m = 1; m < col; ++m)
                    dot += A[r * K + m] * A[col * K + m];
                s -= dot;
            }
            A[r * K + col] = s / d;
        }
    }
    // (the solves run on a local copy: c lives in LDS on the device, and a read-modify-write chain on c.sol was a chain of LDS round
    // trips - cycle counters in k_lm: solve + step 29 % of an LM iteration of a small problem)
    double x[K];
    PL_UNROLL
    for (int i = 0; i < K; ++i)
        x[i] = b[i];
    PL_UNROLL
    for (int i = 0; i < K; ++i) {
        x[i] /= A[i * K + i];
        PL_UNROLL
        for (int r = i + 1; r < K; ++r)
            x[r] -= x[i] * A[r * K + i];
    }
    PL_UNROLL
    for (int i = K - 1; i >= 0; --i) {
        if (i + 1 < K) {
            double dot = A[(i + 1) * K + i] * x[i + 1];
            PL_UNROLL
            for (int j = i + 2; j < K; ++j)
                dot += A[j * K + i] * x[j];
            x[i] -= dot;
        }
        x[i] /= A[i * K + i];
    }
    double sn = 0;
    PL_UNROLL
    for (int i = 0; i < K; ++i) {
        c.sol[i] = x[i];
        sn += x[i] * x[i];
    }
    c.step_norm = sqrt(sn);
    if (c.step_norm < c.opt.step_tol)
        c.done = 1;
}

// After the residual pass on the trial parameters.  Returns true when the step is accepted.
template <int K> PL_HD bool lm_update(LMControl &c, const double *normal, double racc, uint32_t res_count) {
    constexpr int T = NormalSize<K>::kTri;
    c.count = res_count;
    const double cost_new = racc * lm_scale(res_count);
    bool accepted = false;
    bool stop = false;
    if (cost_new < c.cost) {
        const double decrease = c.cost - cost_new;
        accepted = true;
        c.cost = cost_new;
        c.rejac = 1;
        if (c.opt.lambda_update == 0) {
            const double sc = lm_scale(c.count);
            double s = 0;
            PL_UNROLL
            for (int i = 0; i < K; ++i)
                s += c.sol[i] * (c.lambda * c.sol[i] + sc * normal[T + i]);
            const double pred = -s;
            if (pred > 0) {
                const double rho = decrease / pred;
                const double factor = 1.0 - lm_cube(2.0 * rho - 1.0);
                c.lambda *= fmax(1.0 / 3.0, factor);
            } else {
                c.lambda *= 1.0 / 3.0;
            }
            c.nu = 2.0;
        } else {
            c.lambda /= c.opt.lambda_factor;
        }
        c.lambda = fmax(c.opt.min_lambda, c.lambda);
        if (c.cost > 0 && decrease / c.cost < c.opt.relative_cost_tol)
            stop = true;
    } else {
        c.invalid_steps++;
        c.rejac = 0;
        if (c.opt.lambda_update == 0) {
            c.lambda *= c.nu;
            c.nu *= 2.0;
        } else {
            c.lambda *= c.opt.lambda_factor;
        }
        c.lambda = fmin(c.opt.max_lambda, c.lambda);
    }
    if (stop) {
        c.done = 1;
    } else {
        if (c.opt.loss_type == LOSS_TRUNCATED_LE_ZACH)
            c.loss.mu *= 1.5; // bundle.cc:52-75 callback
        c.iterations++;
        if (c.iterations >= c.opt.max_iterations)
            c.done = 1;
    }
    return accepted;
}

// ------------------------------------------------------------------------------------ refiners
// Uniform (per-task) context derived from the current parameters.
struct RefineCtx {
    double M[9];    // R (abs), E (rel), H (hom), F (fund)    row-major
    double G[9];    // adjugate(H) (hom)
    double D[9 * 7]; // d vec(E or F) / d params  (column-major vec index m, D[m*7 + c])
};

template <int EST> struct Refiner;

// ---- absolute pose ----
template <> struct Refiner<EST_ABS> {
    static constexpr int K = 6;
    PL_HD static void prepare(const double *p, RefineCtx &c) {
        Quat q;
        q.w = p[0], q.x = p[1], q.y = p[2], q.z = p[3];
        const Mat3 R = quat_to_rotmat(q);
        PL_UNROLL
        for (int i = 0; i < 9; ++i)
            c.M[i] = R.m[i];
    }
    // returns false when the point is skipped (behind the camera)
    PL_HD static bool residual(const double *p, const RefineCtx &c, const CameraParams &cam, double x, double y,
                               double X, double Y, double Z, double &r0, double &r1) {
        const double *R = c.M;
        const Vec3 Zc = v3(R[0] * X + R[1] * Y + R[2] * Z + p[4], R[3] * X + R[4] * Y + R[5] * Z + p[5],
                           R[6] * X + R[7] * Y + R[8] * Z + p[6]);
        if (Zc.z < 0)
            return false;
        double px, py;
        camera_project(cam, Zc, px, py);
        r0 = px - x;
        r1 = py - y;
        return true;
    }
    PL_HD static bool jacobian(const double *p, const RefineCtx &c, const CameraParams &cam, double x, double y,
                               double X, double Y, double Z, double &r0, double &r1, double *J /*2x6*/) {
        const double *R = c.M;
        const Vec3 Zc = v3(R[0] * X + R[1] * Y + R[2] * Z + p[4], R[3] * X + R[4] * Y + R[5] * Z + p[5],
                           R[6] * X + R[7] * Y + R[8] * Z + p[6]);
        if (Zc.z < 0)
            return false;
        double px, py, Jp[6];
        camera_project_jac(cam, Zc, px, py, Jp);
        r0 = px - x;
        r1 = py - y;
        PL_UNROLL
        for (int a = 0; a < 2; ++a) {
            const double d0 = Jp[3 * a] * R[0] + Jp[3 * a + 1] * R[3] + Jp[3 * a + 2] * R[6];
            const double d1 = Jp[3 * a] * R[1] + Jp[3 * a + 1] * R[4] + Jp[3 * a + 2] * R[7];
            const double d2 = Jp[3 * a] * R[2] + Jp[3 * a + 1] * R[5] + Jp[3 * a + 2] * R[8];
            J[6 * a + 0] = -Z * d1 + Y * d2;
            J[6 * a + 1] = Z * d0 - X * d2;
            J[6 * a + 2] = -Y * d0 + X * d1;
            J[6 * a + 3] = d0;
            J[6 * a + 4] = d1;
            J[6 * a + 5] = d2;
        }
        return true;
    }
    PL_HD static void step(const double *__restrict__ p, const RefineCtx &, const double *__restrict__ dp, double *__restrict__ out) { // (cur, the LM step, trial: never the same storage)
        Quat q;
        q.w = p[0], q.x = p[1], q.y = p[2], q.z = p[3];
        const Quat qn = quat_step_post(q, v3(dp[0], dp[1], dp[2]));
        const Vec3 dt = quat_rotate(q, v3(dp[3], dp[4], dp[5]));
        PL_UNROLL
        for (int i = 0; i < kParamDoubles; ++i)
            out[i] = p[i];
        out[0] = qn.w, out[1] = qn.x, out[2] = qn.y, out[3] = qn.z;
        out[4] = p[4] + dt.x, out[5] = p[5] + dt.y, out[6] = p[6] + dt.z;
    }
};

// Sampson residual and its gradient w.r.t. vec(E) (column-major), shared by E and F refiners
// (optim/relative.h:98-140).
PL_HD double sampson_residual(const double *E, double a0, double a1, double b0, double b1) {
    const double Ea0 = E[0] * a0 + E[1] * a1 + E[2];
    const double Ea1 = E[3] * a0 + E[4] * a1 + E[5];
    const double Ea2 = E[6] * a0 + E[7] * a1 + E[8];
    const double C = b0 * Ea0 + b1 * Ea1 + Ea2;
    const double Eb0 = E[0] * b0 + E[3] * b1 + E[6];
    const double Eb1 = E[1] * b0 + E[4] * b1 + E[7];
    const double n2 = (Ea0 * Ea0 + Ea1 * Ea1) + (Eb0 * Eb0 + Eb1 * Eb1);
    return C / sqrt(n2);
}
PL_HD double sampson_residual_grad(const double *E, double a0, double a1, double b0, double b1, double *dF) {
    const double Ea0 = E[0] * a0 + E[1] * a1 + E[2];
    const double Ea1 = E[3] * a0 + E[4] * a1 + E[5];
    const double Ea2 = E[6] * a0 + E[7] * a1 + E[8];
    const double C = b0 * Ea0 + b1 * Ea1 + Ea2;
    const double J0 = E[0] * b0 + E[3] * b1 + E[6];
    const double J1 = E[1] * b0 + E[4] * b1 + E[7];
    const double J2 = Ea0, J3 = Ea1;
    const double nJ = sqrt(J0 * J0 + J1 * J1 + J2 * J2 + J3 * J3);
    const double inv = 1.0 / nJ;
    const double r = C * inv;
    dF[0] = a0 * b0, dF[1] = a0 * b1, dF[2] = a0;
    dF[3] = a1 * b0, dF[4] = a1 * b1, dF[5] = a1;
    dF[6] = b0, dF[7] = b1, dF[8] = 1.0;
    const double s = C * inv * inv;
    dF[0] -= s * (J2 * a0 + J0 * b0);
    dF[1] -= s * (J3 * a0 + J0 * b1);
    dF[2] -= s * (J0);
    dF[3] -= s * (J2 * a1 + J1 * b0);
    dF[4] -= s * (J3 * a1 + J1 * b1);
    dF[5] -= s * (J1);
    dF[6] -= s * (J2);
    dF[7] -= s * (J3);
    PL_UNROLL
    for (int i = 0; i < 9; ++i)
        dF[i] *= inv;
    return r;
}

// ---- relative pose ----
template <> struct Refiner<EST_REL> {
    static constexpr int K = 5;
    // prepare() also refreshes the tangent basis in the parameter block when `for_jacobian`
    // (the reference sets it up inside compute_jacobian, relative.h:113, and step() reads it).
    PL_HD static void prepare_params(double *p) {
        const Vec3 t = v3(p[4], p[5], p[6]);
        Vec3 tb0;
        if (fabs(t.x) < fabs(t.y))
            tb0 = normalized(cross(t, (fabs(t.x) < fabs(t.z)) ? v3(1, 0, 0) : v3(0, 0, 1)));
        else
            tb0 = normalized(cross(t, (fabs(t.y) < fabs(t.z)) ? v3(0, 1, 0) : v3(0, 0, 1)));
        const Vec3 tb1 = normalized(cross(tb0, t));
        p[7] = tb0.x, p[8] = tb0.y, p[9] = tb0.z;
        p[10] = tb1.x, p[11] = tb1.y, p[12] = tb1.z;
    }
    PL_HD static void prepare(const double *p, RefineCtx &c) {
        Quat q;
        q.w = p[0], q.x = p[1], q.y = p[2], q.z = p[3];
        const Mat3 R = quat_to_rotmat(q);
        const Vec3 t = v3(p[4], p[5], p[6]);
        const Mat3 E = essential_from_motion(R, t);
        PL_UNROLL
        for (int i = 0; i < 9; ++i)
            c.M[i] = E.m[i];
        // D[m][0..2] = d vec(E)/d rot, D[m][3..4] = d vec(E)/d tangent   (relative.h:39-61)
        const Vec3 e0 = col(E, 0), e1 = col(E, 1), e2 = col(E, 2);
        const Vec3 zero = v3(0, 0, 0);
        const Vec3 blocks[3][3] = {{zero, -e2, e1}, {e2, zero, -e0}, {-e1, e0, zero}};
        const Vec3 tb0 = v3(p[7], p[8], p[9]), tb1 = v3(p[10], p[11], p[12]);
        PL_UNROLL
        for (int cb = 0; cb < 3; ++cb) {
            PL_UNROLL
            for (int k = 0; k < 3; ++k) {
                const Vec3 v = blocks[cb][k];
                c.D[(3 * cb + 0) * 7 + k] = v.x;
                c.D[(3 * cb + 1) * 7 + k] = v.y;
                c.D[(3 * cb + 2) * 7 + k] = v.z;
            }
            const Vec3 a = cross(tb0, col(R, cb)), b = cross(tb1, col(R, cb));
            c.D[(3 * cb + 0) * 7 + 3] = a.x, c.D[(3 * cb + 1) * 7 + 3] = a.y, c.D[(3 * cb + 2) * 7 + 3] = a.z;
            c.D[(3 * cb + 0) * 7 + 4] = b.x, c.D[(3 * cb + 1) * 7 + 4] = b.y, c.D[(3 * cb + 2) * 7 + 4] = b.z;
        }
    }
    PL_HD static double residual(const RefineCtx &c, double a0, double a1, double b0, double b1) {
        return sampson_residual(c.M, a0, a1, b0, b1);
    }
    PL_HD static double jacobian(const RefineCtx &c, double a0, double a1, double b0, double b1, double *J) {
        double dF[9];
        const double r = sampson_residual_grad(c.M, a0, a1, b0, b1, dF);
        PL_UNROLL
        for (int k = 0; k < 5; ++k) {
            double s = 0;
            PL_UNROLL
            for (int m = 0; m < 9; ++m)
                s += dF[m] * c.D[m * 7 + k];
            J[k] = s;
        }
        return r;
    }
    PL_HD static void step(const double *__restrict__ p, const RefineCtx &, const double *__restrict__ dp, double *__restrict__ out) { // (cur, the LM step, trial: never the same storage)
        Quat q;
        q.w = p[0], q.x = p[1], q.y = p[2], q.z = p[3];
        const Quat qn = quat_step_post(q, v3(dp[0], dp[1], dp[2]));
        PL_UNROLL
        for (int i = 0; i < kParamDoubles; ++i)
            out[i] = p[i];
        out[0] = qn.w, out[1] = qn.x, out[2] = qn.y, out[3] = qn.z;
        out[4] = p[4] + (p[7] * dp[3] + p[10] * dp[4]);
        out[5] = p[5] + (p[8] * dp[3] + p[11] * dp[4]);
        out[6] = p[6] + (p[9] * dp[3] + p[12] * dp[4]);
    }
};

// ---- relative pose, tangent Sampson (optim/relative.h:168-266, FixCameraRelativePoseRefiner) ----
// Parameters, tangent basis, d vec(E) / d parameters and the step are EST_REL's; a correspondence is the 18 doubles of pl_score.h.
template <> struct Refiner<EST_RELT> {
    static constexpr int K = 5;
    PL_HD static void prepare_params(double *p) { Refiner<EST_REL>::prepare_params(p); }
    PL_HD static void prepare(const double *p, RefineCtx &c) { Refiner<EST_REL>::prepare(p, c); }
    PL_HD static double residual(const RefineCtx &c, const double *pt) { // relative.h:185-191
        double g[4];
        const double C = tangent_sampson_terms(c.M, pt, g);
        const double nJc_sq = (g[2] * g[2] + g[3] * g[3]) + (g[0] * g[0] + g[1] * g[1]);
        return C / sqrt(nJc_sq);
    }
    PL_HD static double jacobian(const RefineCtx &c, const double *pt, double *J) { // relative.h:207-247
        const double *d1 = pt, *d2 = pt + 3, *M1 = pt + 6, *M2 = pt + 12;
        double g[4]; // J_C
        const double C = tangent_sampson_terms(c.M, pt, g);
        const double nJ = sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2] + g[3] * g[3]);
        const double inv = 1.0 / nJ;
        const double r = C * inv;
        const double s = C * inv * inv;
        double dF[9];
        PL_UNROLL
        for (int i = 0; i < 3; ++i)
            PL_UNROLL
            for (int j = 0; j < 3; ++j) {
                double f = d1[i] * d2[j];
                f -= s * (g[0] * M1[2 * i] * d2[j] + g[1] * M1[2 * i + 1] * d2[j] + g[2] * M2[2 * j] * d1[i] + g[3] * M2[2 * j + 1] * d1[i]);
                dF[3 * i + j] = f * inv;
            }
        PL_UNROLL
        for (int k = 0; k < 5; ++k) {
            double a = 0;
            PL_UNROLL
            for (int m = 0; m < 9; ++m)
                a += dF[m] * c.D[m * 7 + k];
            J[k] = a;
        }
        return r;
    }
    PL_HD static void step(const double *__restrict__ p, const RefineCtx &c, const double *__restrict__ dp, double *__restrict__ out) {
        Refiner<EST_REL>::step(p, c, dp, out);
    }
};

// ---- absolute pose of a 1D-radial camera (optim/absolute.h:342-409, Radial1DAbsolutePoseRefiner; camera parameters {0, 0}) ----
// Five parameters: rotation (pre-multiplied step, quat_step_pre) and t_x, t_y; t_z is never touched.  The projection is the unit
// vector of the first two coordinates (camera_models.cc:2288-2313), the residual alpha xp - x with alpha = xp . x; terms with
// alpha < 0 are skipped (the scorer's test is alpha > 0: both as in the reference).  The residual takes Z = q X q* + t
// (CameraPose::apply), the Jacobian Z = R(q) X + t, as the reference does.  Same call shape as Refiner<EST_ABS> (`cam` is not read).
template <> struct Refiner<EST_RAD1D> {
    static constexpr int K = 5;
    PL_HD static void prepare(const double *p, RefineCtx &c) { Refiner<EST_ABS>::prepare(p, c); }
    PL_HD static bool residual(const double *p, const RefineCtx &, const CameraParams &, double x, double y, double X, double Y,
                               double Z, double &r0, double &r1) {
        Quat q;
        q.w = p[0], q.x = p[1], q.y = p[2], q.z = p[3];
        const Vec3 Zc = quat_rotate(q, v3(X, Y, Z)) + v3(p[4], p[5], p[6]);
        const double n = sqrt(0.0 + Zc.x * Zc.x + Zc.y * Zc.y);
        const double nrm = n < 1e-8 ? 1e-8 : n;
        const double v0 = Zc.x / nrm, v1 = Zc.y / nrm;
        const double alpha = 0.0 + v0 * x + v1 * y;
        if (alpha < 0)
            return false;
        r0 = alpha * v0 - x;
        r1 = alpha * v1 - y;
        return true;
    }
    PL_HD static bool jacobian(const double *p, const RefineCtx &c, const CameraParams &, double x, double y, double X, double Y,
                               double Z, double &r0, double &r1, double *J /*2x5*/) {
        const double *R = c.M;
        const double RX0 = R[0] * X + R[1] * Y + R[2] * Z, RX1 = R[3] * X + R[4] * Y + R[5] * Z, RX2 = R[6] * X + R[7] * Y + R[8] * Z;
        const double Z0 = RX0 + p[4], Z1 = RX1 + p[5];
        const double n = sqrt(0.0 + Z0 * Z0 + Z1 * Z1);
        const double nrm = n < 1e-8 ? 1e-8 : n;
        const double v0 = Z0 / nrm, v1 = Z1 / nrm;
        // (I - v v^T) / |z|
        const double P00 = (1.0 - v0 * v0) / nrm, P01 = (0.0 - v0 * v1) / nrm, P10 = (0.0 - v1 * v0) / nrm, P11 = (1.0 - v1 * v1) / nrm;
        const double alpha = 0.0 + v0 * x + v1 * y;
        if (alpha < 0)
            return false;
        r0 = alpha * v0 - x;
        r1 = alpha * v1 - y;
        // d r / d z = (xp x^T + alpha I) (I - v v^T) / |z|, then d z / d (rotation, t_x, t_y)   (absolute.h:382-386)
        const double B00 = v0 * x + alpha * 1.0, B01 = v0 * y + alpha * 0.0, B10 = v1 * x + alpha * 0.0, B11 = v1 * y + alpha * 1.0;
        const double D[4] = {B00 * P00 + B01 * P10, B00 * P01 + B01 * P11, B10 * P00 + B11 * P10, B10 * P01 + B11 * P11};
        PL_UNROLL
        for (int a = 0; a < 2; ++a) {
            const double d0 = D[2 * a], d1 = D[2 * a + 1];
            J[5 * a + 0] = d0 * 0.0 + d1 * -RX2;
            J[5 * a + 1] = d0 * RX2 + d1 * 0.0;
            J[5 * a + 2] = d0 * -RX1 + d1 * RX0;
            J[5 * a + 3] = d0 * 1.0 + d1 * 0.0;
            J[5 * a + 4] = d0 * 0.0 + d1 * 1.0;
        }
        return true;
    }
    PL_HD static void step(const double *__restrict__ p, const RefineCtx &, const double *__restrict__ dp, double *__restrict__ out) {
        Quat q;
        q.w = p[0], q.x = p[1], q.y = p[2], q.z = p[3];
        const Quat qn = quat_step_pre(q, v3(dp[0], dp[1], dp[2]));
        PL_UNROLL
        for (int i = 0; i < kParamDoubles; ++i)
            out[i] = p[i];
        out[0] = qn.w, out[1] = qn.x, out[2] = qn.y, out[3] = qn.z;
        out[4] = p[4] + dp[3], out[5] = p[5] + dp[4];
    }
};

// ---- homography ----
template <> struct Refiner<EST_HOM> {
    static constexpr int K = 8;
    PL_HD static void prepare(const double *p, RefineCtx &c) {
        const double *H = p;
        PL_UNROLL
        for (int i = 0; i < 9; ++i)
            c.M[i] = H[i];
        c.G[0] = H[4] * H[8] - H[5] * H[7];
        c.G[1] = H[2] * H[7] - H[1] * H[8];
        c.G[2] = H[1] * H[5] - H[2] * H[4];
        c.G[3] = H[5] * H[6] - H[3] * H[8];
        c.G[4] = H[0] * H[8] - H[2] * H[6];
        c.G[5] = H[2] * H[3] - H[0] * H[5];
        c.G[6] = H[3] * H[7] - H[4] * H[6];
        c.G[7] = H[1] * H[6] - H[0] * H[7];
        c.G[8] = H[0] * H[4] - H[1] * H[3];
    }
    PL_HD static void transfer(const double *H, double a0, double a1, double &z0, double &z1, double &inv) {
        const double h0 = H[0] * a0 + H[1] * a1 + H[2];
        const double h1 = H[3] * a0 + H[4] * a1 + H[5];
        inv = 1.0 / (H[6] * a0 + H[7] * a1 + H[8]);
        z0 = h0 * inv;
        z1 = h1 * inv;
    }
    // forward residual (f0,f1) and backward residual (g0,g1)
    PL_HD static void residual(const RefineCtx &c, double a0, double a1, double b0, double b1, double &f0, double &f1,
                               double &g0, double &g1) {
        double z0, z1, inv;
        transfer(c.M, a0, a1, z0, z1, inv);
        f0 = z0 - b0, f1 = z1 - b1;
        transfer(c.G, b0, b1, z0, z1, inv);
        g0 = z0 - a0, g1 = z1 - a1;
    }
    PL_HD static void jacobian(const RefineCtx &c, double a0, double a1, double b0, double b1, double &f0, double &f1,
                               double *Jf /*2x8*/, double &g0, double &g1, double *Jb /*2x8*/) {
        const double *H = c.M;
        double z0, z1, inv;
        transfer(H, a0, a1, z0, z1, inv);
        f0 = z0 - b0, f1 = z1 - b1;
        const double jf[16] = {a0, 0.0, -a0 * z0, a1, 0.0, -a1 * z0, 1.0, 0.0, 0.0, a0, -a0 * z1, 0.0, a1, -a1 * z1, 0.0, 1.0};
        PL_UNROLL
        for (int i = 0; i < 16; ++i)
            Jf[i] = jf[i] * inv;
        double y0, y1, ginv;
        transfer(c.G, b0, b1, y0, y1, ginv);
        g0 = y0 - a0, g1 = y1 - a1;
        const double H00 = H[0], H01 = H[1], H02 = H[2], H10 = H[3], H11 = H[4], H12 = H[5], H20 = H[6], H21 = H[7],
                     H22 = H[8];
        const double y0b1 = y0 * b1, y0b0 = y0 * b0, y1b1 = y1 * b1, y1b0 = y1 * b0;
        const double jb[16] = {H21 * y0b1 - H11 * y0,
                               H01 * y0 - H21 * y0b0,
                               H11 * y0b0 - H01 * y0b1,
                               H12 - H22 * b1 + H10 * y0 - H20 * y0b1,
                               H22 * b0 - H02 - H00 * y0 + H20 * y0b0,
                               H02 * b1 - H12 * b0 + H00 * y0b1 - H10 * y0b0,
                               H21 * b1 - H11,
                               H01 - H21 * b0,
                               H22 * b1 - H12 - H11 * y1 + H21 * y1b1,
                               H02 - H22 * b0 + H01 * y1 - H21 * y1b0,
                               H12 * b0 - H02 * b1 - H01 * y1b1 + H11 * y1b0,
                               H10 * y1 - H20 * y1b1,
                               H20 * y1b0 - H00 * y1,
                               H00 * y1b1 - H10 * y1b0,
                               H10 - H20 * b1,
                               H20 * b0 - H00};
        PL_UNROLL
        for (int i = 0; i < 16; ++i)
            Jb[i] = jb[i] * ginv;
    }
    PL_HD static void step(const double *__restrict__ p, const RefineCtx &, const double *__restrict__ dp, double *__restrict__ out) { // (cur, the LM step, trial: never the same storage)
        PL_UNROLL
        for (int i = 0; i < kParamDoubles; ++i)
            out[i] = p[i];
        // parameters = first 8 entries of column-major H: e -> (row e%3, col e/3)
        PL_UNROLL
        for (int e = 0; e < 8; ++e)
            out[3 * (e % 3) + (e / 3)] = p[3 * (e % 3) + (e / 3)] + dp[e];
    }
};

// ---- fundamental matrix (factorised) ----
PL_HD void factorized_F(const double *p, double *F) { // optim_utils.h:73-77
    Quat qU, qV;
    qU.w = p[0], qU.x = p[1], qU.y = p[2], qU.z = p[3];
    qV.w = p[4], qV.x = p[5], qV.y = p[6], qV.z = p[7];
    const Mat3 U = quat_to_rotmat(qU), V = quat_to_rotmat(qV);
    const double sigma = p[8];
    PL_UNROLL
    for (int i = 0; i < 3; ++i)
        PL_UNROLL
        for (int j = 0; j < 3; ++j)
            F[3 * i + j] = U.m[3 * i] * V.m[3 * j] + (sigma * U.m[3 * i + 1]) * V.m[3 * j + 1];
}
template <> struct Refiner<EST_FUND> {
    static constexpr int K = 7;
    PL_HD static void prepare(const double *p, RefineCtx &c) {
        factorized_F(p, c.M);
        Quat qU, qV;
        qU.w = p[0], qU.x = p[1], qU.y = p[2], qU.z = p[3];
        qV.w = p[4], qV.x = p[5], qV.y = p[6], qV.z = p[7];
        const Mat3 U = quat_to_rotmat(qU), V = quat_to_rotmat(qV);
        Mat3 F;
        PL_UNROLL
        for (int i = 0; i < 9; ++i)
            F.m[i] = c.M[i];
        const Vec3 axes[3] = {v3(1, 0, 0), v3(0, 1, 0), v3(0, 0, 1)};
        PL_UNROLL
        for (int cb = 0; cb < 3; ++cb) {
            const Vec3 f = col(F, cb);
            PL_UNROLL
            for (int k = 0; k < 3; ++k) {
                const Vec3 d = cross(axes[k], f);
                c.D[(3 * cb + 0) * 7 + k] = d.x, c.D[(3 * cb + 1) * 7 + k] = d.y, c.D[(3 * cb + 2) * 7 + k] = d.z;
            }
        }
        PL_UNROLL
        for (int r = 0; r < 3; ++r) {
            const Vec3 f = row(F, r);
            PL_UNROLL
            for (int k = 0; k < 3; ++k) {
                const Vec3 d = cross(axes[k], f);
                c.D[(0 + r) * 7 + 3 + k] = d.x, c.D[(3 + r) * 7 + 3 + k] = d.y, c.D[(6 + r) * 7 + 3 + k] = d.z;
            }
        }
        PL_UNROLL
        for (int j = 0; j < 3; ++j)
            PL_UNROLL
            for (int i = 0; i < 3; ++i)
                c.D[(3 * j + i) * 7 + 6] = U.m[3 * i + 1] * V.m[3 * j + 1];
    }
    PL_HD static double residual(const RefineCtx &c, double a0, double a1, double b0, double b1) {
        return sampson_residual(c.M, a0, a1, b0, b1);
    }
    PL_HD static double jacobian(const RefineCtx &c, double a0, double a1, double b0, double b1, double *J) {
        double dF[9];
        const double r = sampson_residual_grad(c.M, a0, a1, b0, b1, dF);
        PL_UNROLL
        for (int k = 0; k < 7; ++k) {
            double s = 0;
            PL_UNROLL
            for (int m = 0; m < 9; ++m)
                s += dF[m] * c.D[m * 7 + k];
            J[k] = s;
        }
        return r;
    }
    PL_HD static void step(const double *__restrict__ p, const RefineCtx &, const double *__restrict__ dp, double *__restrict__ out) { // (cur, the LM step, trial: never the same storage)
        Quat qU, qV;
        qU.w = p[0], qU.x = p[1], qU.y = p[2], qU.z = p[3];
        qV.w = p[4], qV.x = p[5], qV.y = p[6], qV.z = p[7];
        const Quat u = quat_step_pre(qU, v3(dp[0], dp[1], dp[2]));
        const Quat v = quat_step_pre(qV, v3(dp[3], dp[4], dp[5]));
        PL_UNROLL
        for (int i = 0; i < kParamDoubles; ++i)
            out[i] = p[i];
        out[0] = u.w, out[1] = u.x, out[2] = u.y, out[3] = u.z;
        out[4] = v.w, out[5] = v.x, out[6] = v.y, out[7] = v.z;
        out[8] = p[8] + dp[6];
    }
};

// Record (what the scorers consume) of a refined parameter block: pose (q, t) for the absolute / relative problems,
// H row-major, or the Bartoli-Sturm factorisation of F (optim_utils.h:73-77).  est: pl_score.h Estimator.
PL_HD void record_from_lm_params(int est, const double *params, double *rec) {
    if (est == 0 || est == 1 || est == 4 || est == 5) {
        Quat q;
        q.w = params[0], q.x = params[1], q.y = params[2], q.z = params[3];
        store_pose_model_q(rec, q, v3(params[4], params[5], params[6]), est == 1 || est == 4);
    } else if (est == 3) {
        Mat3 H;
        for (int i = 0; i < 9; ++i)
            H.m[i] = params[i];
        store_matrix_model(rec, H);
    } else {
        Mat3 F;
        factorized_F(params, F.m);
        store_matrix_model(rec, F);
    }
}

} // namespace pl
