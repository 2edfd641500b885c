// TEST-ONLY C interface to the reference's tangent-Sampson relative-pose path, for tests/golden/make_golden_tangent.py and the
// fixture-against-live-reference test.  Compiled against the reference's headers where they lie and linked to
// oracle/_ref/libposelib_ref.so (whose C shim, oracle/ref_shim/ref_api.cc, does not pass RelativePoseOptions::tangent_sampson).
// Built into a temporary directory by tests/ref_tangent_lib.py; nothing compiled from it is kept.
#include <PoseLib/misc/camera_models.h>
#include <PoseLib/robust.h>
#include <PoseLib/robust/bundle.h>
#include <PoseLib/robust/utils.h>

#include <cstdint>
#include <vector>

using namespace poselib;

namespace {
Camera make_camera(int model_id, const double *params, int num_params) {
    Camera c;
    c.model_id = model_id;
    c.width = c.height = 1000;
    c.params.assign(params, params + num_params);
    return c;
}
struct Bearings {
    std::vector<Point3D> d1, d2;
    std::vector<Eigen::Matrix<double, 3, 2>> M1, M2;
    Bearings(const double *pd1, const double *pd2, const double *pM1, const double *pM2, uint32_t n) : d1(n), d2(n), M1(n), M2(n) {
        for (uint32_t i = 0; i < n; ++i) {
            d1[i] = Point3D(pd1[3 * i], pd1[3 * i + 1], pd1[3 * i + 2]);
            d2[i] = Point3D(pd2[3 * i], pd2[3 * i + 1], pd2[3 * i + 2]);
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 2; ++c) {
                    M1[i](r, c) = pM1[6 * i + 2 * r + c];
                    M2[i](r, c) = pM2[6 * i + 2 * r + c];
                }
        }
    }
};
CameraPose make_pose(const double *p7) {
    CameraPose p;
    p.q = Eigen::Vector4d(p7[0], p7[1], p7[2], p7[3]);
    p.t = Eigen::Vector3d(p7[4], p7[5], p7[6]);
    return p;
}
void store_pose(const CameraPose &p, double *p7) {
    for (int i = 0; i < 4; ++i)
        p7[i] = p.q(i);
    for (int i = 0; i < 3; ++i)
        p7[4 + i] = p.t(i);
}
} // namespace

extern "C" {

double rt_focal(int model_id, const double *params, int num_params) { return make_camera(model_id, params, num_params).focal(); }

void rt_rescale(int model_id, const double *params, int num_params, double scale, double *out) {
    Camera c = make_camera(model_id, params, num_params);
    c.rescale(scale);
    for (int i = 0; i < num_params; ++i)
        out[i] = c.params[i];
}

// Camera::unproject_with_jac per pixel: d (n x 3), M (n x 6, 3x2 row-major), det(J J^T) of the projection's Jacobian at d
void rt_unproject_with_jac(int model_id, const double *params, int num_params, const double *pix, uint32_t n, double *d, double *M,
                           double *det) {
    const Camera c = make_camera(model_id, params, num_params);
    for (uint32_t i = 0; i < n; ++i) {
        Eigen::Vector3d x;
        Eigen::Matrix<double, 3, 2> J;
        c.unproject_with_jac(Eigen::Vector2d(pix[2 * i], pix[2 * i + 1]), &x, &J);
        for (int r = 0; r < 3; ++r) {
            d[3 * i + r] = x(r);
            M[6 * i + 2 * r] = J(r, 0);
            M[6 * i + 2 * r + 1] = J(r, 1);
        }
        Eigen::Vector2d xp;
        Eigen::Matrix<double, 2, 3> jp;
        c.project_with_jac(x, &xp, &jp);
        const Eigen::Matrix2d B = jp * jp.transpose();
        det[i] = B(0, 0) * B(1, 1) - B(0, 1) * B(1, 0);
    }
}

// compute_tangent_sampson_msac_score + get_tangent_sampson_inliers of a pose on prepared bearings
double rt_score(const double *pose7, const double *d1, const double *d2, const double *M1, const double *M2, uint32_t n, double thr2,
                uint64_t *count, uint8_t *mask, uint64_t *mask_count) {
    const Bearings b(d1, d2, M1, M2, n);
    const CameraPose pose = make_pose(pose7);
    size_t cnt = 0;
    const double score = compute_tangent_sampson_msac_score(pose, b.d1, b.d2, b.M1, b.M2, thr2, &cnt);
    *count = cnt;
    std::vector<char> inl;
    *mask_count = (uint64_t)get_tangent_sampson_inliers(pose, b.d1, b.d2, b.M1, b.M2, thr2, &inl);
    for (uint32_t i = 0; i < n; ++i)
        mask[i] = inl[i] ? 1 : 0;
    return score;
}

// refine_relpose(d1, d2, M1, M2, pose, opt): pose in / out; out3 = iterations, initial cost, cost
void rt_refine(const double *d1, const double *d2, const double *M1, const double *M2, uint32_t n, double *pose7, int loss_type,
               double loss_scale, uint64_t max_iterations, double *out3) {
    const Bearings b(d1, d2, M1, M2, n);
    CameraPose pose = make_pose(pose7);
    BundleOptions o;
    o.loss_type = (BundleOptions::LossType)loss_type;
    o.loss_scale = loss_scale;
    o.max_iterations = max_iterations;
    const BundleStats st = refine_relpose(b.d1, b.d2, b.M1, b.M2, &pose, o);
    store_pose(pose, pose7);
    out3[0] = (double)st.iterations, out3[1] = st.initial_cost, out3[2] = st.cost;
}

// estimate_relative_pose(x1, x2, camera1, camera2, opt, &pose, &inliers).  A camera with model_id -1 is the identity camera.
// iopt: max_iterations, min_iterations, seed, progressive_sampling, score_initial_model, tangent_sampson, bundle loss type,
// bundle max_iterations;  dopt: max_error, success_prob, bundle loss_scale.  stats5: refinements, iterations, num_inliers,
// inlier_ratio, model_score
void rt_estimate(const double *x1, const double *x2, uint32_t n, int model1, const double *params1, int np1, int model2,
                 const double *params2, int np2, const uint64_t *iopt, const double *dopt, double *pose7, uint8_t *mask,
                 double *stats5) {
    std::vector<Point2D> a(n), b(n);
    for (uint32_t i = 0; i < n; ++i) {
        a[i] = Point2D(x1[2 * i], x1[2 * i + 1]);
        b[i] = Point2D(x2[2 * i], x2[2 * i + 1]);
    }
    RelativePoseOptions o;
    o.ransac.max_iterations = iopt[0];
    o.ransac.min_iterations = iopt[1];
    o.ransac.seed = iopt[2];
    o.ransac.progressive_sampling = iopt[3] != 0;
    o.ransac.score_initial_model = iopt[4] != 0;
    o.tangent_sampson = iopt[5] != 0;
    o.bundle.loss_type = (BundleOptions::LossType)iopt[6];
    o.bundle.max_iterations = iopt[7];
    o.max_error = dopt[0];
    o.ransac.success_prob = dopt[1];
    o.bundle.loss_scale = dopt[2];
    CameraPose pose = make_pose(pose7);
    std::vector<char> inl;
    const RansacStats st =
        estimate_relative_pose(a, b, make_camera(model1, params1, np1), make_camera(model2, params2, np2), o, &pose, &inl);
    store_pose(pose, pose7);
    for (uint32_t i = 0; i < n; ++i)
        mask[i] = (i < inl.size() && inl[i]) ? 1 : 0;
    stats5[0] = (double)st.refinements, stats5[1] = (double)st.iterations, stats5[2] = (double)st.num_inliers;
    stats5[3] = st.inlier_ratio, stats5[4] = st.model_score;
}
}
