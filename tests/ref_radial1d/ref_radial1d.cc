// TEST-ONLY stand-alone driver of the reference's 1D-radial absolute-pose path, for tests/golden/make_golden_radial1d.py.
// A program of its own, run as a child process with binary files of doubles in and out (tests/ref_radial1d_lib.py): it is compiled
// against the reference's headers where they lie, TOGETHER with the reference's solvers/p5lp_radial.cc compiled in place - the
// reference library under oracle/_ref was built without that file and only traps there - and an executable's own definitions are
// the ones the dynamic linker binds first, whatever else the process loads.  Nothing compiled from it is kept.
//   ref_radial1d selftest                 p5lp_radial on a fixed sample (a trap shows as the exit status)
//   ref_radial1d <command> <in> <out>     commands and record layouts below
#include <PoseLib/robust.h>
#include <PoseLib/robust/bundle.h>
#include <PoseLib/robust/ransac.h>
#include <PoseLib/robust/utils.h>
#include <PoseLib/solvers/p5lp_radial.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace poselib;

namespace {
std::vector<double> read_doubles(const char *path) {
    std::vector<double> v;
    FILE *f = std::fopen(path, "rb");
    if (!f)
        return v;
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    v.resize((size_t)bytes / sizeof(double));
    if (std::fread(v.data(), sizeof(double), v.size(), f) != v.size())
        v.clear();
    std::fclose(f);
    return v;
}
bool write_doubles(const char *path, const std::vector<double> &v) {
    FILE *f = std::fopen(path, "wb");
    if (!f)
        return false;
    const bool ok = std::fwrite(v.data(), sizeof(double), v.size(), f) == v.size();
    std::fclose(f);
    return ok;
}
CameraPose make_pose(const double *p7) {
    CameraPose p;
    p.q = Eigen::Vector4d(p7[0], p7[1], p7[2], p7[3]);
    p.t = Eigen::Vector3d(p7[4], p7[5], p7[6]);
    return p;
}
void push_pose(std::vector<double> &out, const CameraPose &p) {
    for (int i = 0; i < 4; ++i)
        out.push_back(p.q(i));
    for (int i = 0; i < 3; ++i)
        out.push_back(p.t(i));
}
void points(const double *x, const double *X, size_t n, std::vector<Point2D> &a, std::vector<Point3D> &b) {
    a.resize(n), b.resize(n);
    for (size_t i = 0; i < n; ++i) {
        a[i] = Point2D(x[2 * i], x[2 * i + 1]);
        b[i] = Point3D(X[3 * i], X[3 * i + 1], X[3 * i + 2]);
    }
}

// in: S, then per sample x (5 x 2) and X (5 x 3).  out per sample: return value, output size, 4 poses of 7 (zeros beyond the size)
std::vector<double> cmd_solve(const std::vector<double> &in) {
    const size_t S = (size_t)in[0];
    std::vector<double> out;
    for (size_t s = 0; s < S; ++s) {
        const double *p = &in[1 + 25 * s];
        std::vector<Eigen::Vector2d> x(5);
        std::vector<Eigen::Vector3d> X(5);
        for (int i = 0; i < 5; ++i) {
            x[i] = Eigen::Vector2d(p[2 * i], p[2 * i + 1]);
            X[i] = Eigen::Vector3d(p[10 + 3 * i], p[10 + 3 * i + 1], p[10 + 3 * i + 2]);
        }
        std::vector<CameraPose> poses;
        const int ret = p5lp_radial(x, X, &poses);
        out.push_back(ret);
        out.push_back((double)poses.size());
        for (size_t m = 0; m < 4; ++m)
            if (m < poses.size())
                push_pose(out, poses[m]);
            else
                out.insert(out.end(), 7, 0.0);
    }
    return out;
}

// Radial1DAbsolutePoseEstimator::generate_models (estimators/absolute_pose.cc:353-361) on given samples instead of drawn ones: the
// sample's 2-D points through .normalized(), then p5lp_radial.
// in: n, S, x (n x 2), X (n x 3), S samples of 5 indices.  out per sample: output size, 4 poses of 7 (zeros beyond the size)
std::vector<double> cmd_generate(const std::vector<double> &in) {
    const size_t n = (size_t)in[0], S = (size_t)in[1];
    std::vector<Point2D> x;
    std::vector<Point3D> X;
    points(&in[2], &in[2 + 2 * n], n, x, X);
    const double *idx = &in[2 + 5 * n];
    std::vector<double> out;
    for (size_t s = 0; s < S; ++s) {
        std::vector<Eigen::Vector2d> xs(5);
        std::vector<Eigen::Vector3d> Xs(5);
        for (int k = 0; k < 5; ++k) {
            const size_t i = (size_t)idx[5 * s + k];
            xs[k] = x[i].normalized();
            Xs[k] = X[i];
        }
        std::vector<CameraPose> poses;
        p5lp_radial(xs, Xs, &poses);
        out.push_back((double)poses.size());
        for (size_t m = 0; m < 4; ++m)
            if (m < poses.size())
                push_pose(out, poses[m]);
            else
                out.insert(out.end(), 7, 0.0);
    }
    return out;
}

// in: n, thr2, pose (7), x (n x 2), X (n x 3).  out: score, count, mask (n)
std::vector<double> cmd_score(const std::vector<double> &in) {
    const size_t n = (size_t)in[0];
    std::vector<Point2D> x;
    std::vector<Point3D> X;
    points(&in[9], &in[9 + 2 * n], n, x, X);
    const CameraPose pose = make_pose(&in[2]);
    size_t cnt = 0;
    const double score = compute_msac_score_1D_radial(pose, x, X, in[1], &cnt);
    std::vector<char> inl;
    get_inliers_1D_radial(pose, x, X, in[1], &inl);
    std::vector<double> out = {score, (double)cnt};
    for (size_t i = 0; i < n; ++i)
        out.push_back(inl[i] ? 1.0 : 0.0);
    return out;
}

// in: n, loss type, loss scale, max iterations, pose (7), x, X.  out: pose (7), iterations, initial cost, cost
std::vector<double> cmd_refine(const std::vector<double> &in) {
    const size_t n = (size_t)in[0];
    std::vector<Point2D> x;
    std::vector<Point3D> X;
    points(&in[11], &in[11 + 2 * n], n, x, X);
    CameraPose pose = make_pose(&in[4]);
    BundleOptions o;
    o.loss_type = (BundleOptions::LossType)(int)in[1];
    o.loss_scale = in[2];
    o.max_iterations = (size_t)in[3];
    Camera camera(Radial1DCameraModel::model_id, {0.0, 0.0});
    const BundleStats st = bundle_adjust_1D_radial(x, X, &pose, camera, o);
    std::vector<double> out;
    push_pose(out, pose);
    out.push_back((double)st.iterations), out.push_back(st.initial_cost), out.push_back(st.cost);
    return out;
}

// in: n, max_iterations, min_iterations, seed, progressive_sampling, score_initial_model, bundle loss type, bundle max_iterations,
// max_error, success_prob, bundle loss_scale, pose (7), x, X.  out: pose (7), refinements, iterations, num_inliers, inlier_ratio,
// model_score, mask (n)
std::vector<double> cmd_estimate(const std::vector<double> &in, bool front_end) {
    const size_t n = (size_t)in[0];
    std::vector<Point2D> x;
    std::vector<Point3D> X;
    points(&in[18], &in[18 + 2 * n], n, x, X);
    AbsolutePoseOptions o;
    o.ransac.max_iterations = (size_t)in[1];
    o.ransac.min_iterations = (size_t)in[2];
    o.ransac.seed = (unsigned long)in[3];
    o.ransac.progressive_sampling = in[4] != 0;
    o.ransac.score_initial_model = in[5] != 0;
    o.bundle.loss_type = (BundleOptions::LossType)(int)in[6];
    o.bundle.max_iterations = (size_t)in[7];
    o.max_error = in[8];
    o.ransac.success_prob = in[9];
    o.bundle.loss_scale = in[10];
    CameraPose pose = make_pose(&in[11]);
    std::vector<char> inl;
    const RansacStats st = front_end ? estimate_1D_radial_absolute_pose(x, X, o, &pose, &inl) : ransac_1D_radial_pnp(x, X, o, &pose, &inl);
    std::vector<double> out;
    push_pose(out, pose);
    out.push_back((double)st.refinements), out.push_back((double)st.iterations), out.push_back((double)st.num_inliers);
    out.push_back(st.inlier_ratio), out.push_back(st.model_score);
    for (size_t i = 0; i < n; ++i)
        out.push_back((i < inl.size() && inl[i]) ? 1.0 : 0.0);
    return out;
}
} // namespace

int main(int argc, char **argv) {
    if (argc == 2 && std::string(argv[1]) == "selftest") {
        std::vector<Eigen::Vector2d> x = {{0.6, 0.8}, {-0.8, 0.6}, {0.28, -0.96}, {1.0, 0.0}, {-0.6, -0.8}};
        std::vector<Eigen::Vector3d> X = {{1, 2, 5}, {-2, 1, 6}, {0.5, -3, 4}, {3, 0.2, 7}, {-1, -2, 5.5}};
        std::vector<CameraPose> poses;
        const int ret = p5lp_radial(x, X, &poses);
        std::printf("selftest %d %zu\n", ret, poses.size());
        return 0;
    }
    if (argc != 4)
        return 2;
    const std::vector<double> in = read_doubles(argv[2]);
    if (in.empty())
        return 3;
    const std::string cmd = argv[1];
    std::vector<double> out;
    if (cmd == "solve")
        out = cmd_solve(in);
    else if (cmd == "generate")
        out = cmd_generate(in);
    else if (cmd == "score")
        out = cmd_score(in);
    else if (cmd == "refine")
        out = cmd_refine(in);
    else if (cmd == "estimate")
        out = cmd_estimate(in, true);
    else if (cmd == "ransac")
        out = cmd_estimate(in, false);
    else
        return 2;
    return write_doubles(argv[3], out) ? 0 : 4;
}
