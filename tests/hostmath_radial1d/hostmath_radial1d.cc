// TEST-ONLY host compilation of the 1D-radial path of the device headers (poselib_amd/csrc/pl_solver_p5lp_radial.h, pl_score.h,
// pl_prefilter.h, pl_refine.h): the minimal solver, the exact score and mask, the fp32 pre-filter and the refiner, so that the CPU
// suite can hold them to the reference's recorded outputs bit for bit.  Never used by the product.
#include "../../poselib_amd/csrc/pl_prefilter.h"
#include "../../poselib_amd/csrc/pl_refine.h"
#include "../../poselib_amd/csrc/pl_score.h"
#include "../../poselib_amd/csrc/pl_solver_p5lp_radial.h"

#include <cstdint>
#include <cstring>

using namespace pl;

extern "C" {

// p5lp_radial_emit per sample: xs (S x 5 x 2), Xs (S x 5 x 3) -> counts (S), poses (S x 4 x 7: q, t as the record holds them),
// nan (S x 4: the record's NaN flag)
void rd_p5lp(const double *xs, const double *Xs, uint32_t S, uint32_t *counts, double *poses, uint8_t *nan) {
    for (uint32_t s = 0; s < S; ++s) {
        double x[5][2], X[5][3];
        for (int i = 0; i < 5; ++i) {
            x[i][0] = xs[10 * s + 2 * i], x[i][1] = xs[10 * s + 2 * i + 1];
            for (int k = 0; k < 3; ++k)
                X[i][k] = Xs[15 * s + 3 * i + k];
        }
        counts[s] = (uint32_t)p5lp_radial_emit(x, X, [&](int m, const Mat3 &R, const Vec3 &t) {
            double rec[kModelStride];
            nan[4 * s + m] = store_pose_model(rec, R, t, false) ? 1 : 0;
            std::memcpy(poses + 28 * s + 7 * m, rec, sizeof(double) * 7);
        });
    }
}

// the generator's normalisation of a sample point (absolute_pose.cc:357)
void rd_normalized2(const double *x, uint32_t n, double *out) {
    for (uint32_t i = 0; i < n; ++i)
        normalized2(x[2 * i], x[2 * i + 1], out[2 * i], out[2 * i + 1]);
}

// the record of a pose as the scorers read it, then score / count / mask in correspondence order (k_score_seq<EST_RAD1D>, k_mask<EST_RAD1D>)
double rd_score(const double *pose7, const double *x, const double *X, uint32_t n, double thr2, uint64_t *count, uint8_t *mask) {
    double rec[kModelStride];
    Quat q;
    q.w = pose7[0], q.x = pose7[1], q.y = pose7[2], q.z = pose7[3];
    store_pose_model_q(rec, q, v3(pose7[4], pose7[5], pose7[6]), false);
    double score = 0;
    *count = 0;
    for (uint32_t i = 0; i < n; ++i) {
        double r2;
        const bool in = radial1d_inlier(rec, x[2 * i], x[2 * i + 1], X[3 * i], X[3 * i + 1], X[3 * i + 2], thr2, r2);
        score += in ? r2 : thr2;
        *count += in;
        if (mask)
            mask[i] = in;
    }
    return score;
}

// The fp32 pre-filter of k_score_radial1d next to the exact decision for a pose: rejected[i] = the filter's verdict "certainly not an
// inlier" as the kernel forms it; inlier[i] = the exact r^2 < thr2 && alpha > 0.  Returns 0 when the model is skipped (a NaN among the entries read),
// 2 when it lies outside the filter's range (every point exact), 1 otherwise.
int rd_prefilter(const double *pose7, const double *x, const double *X, uint32_t n, double thr2, uint8_t *rejected, uint8_t *inlier) {
    double rec[kModelStride];
    Quat q;
    q.w = pose7[0], q.x = pose7[1], q.y = pose7[2], q.z = pose7[3];
    store_pose_model_q(rec, q, v3(pose7[4], pose7[5], pose7[6]), false);
    const float *r = reinterpret_cast<const float *>(rec + kShadowOff);
    // the kernel's entry test: a NaN among the eight entries the score reads (not the record's flag, which also covers the third
    // row of R and t_z)
    const bool nanflag = (r[0] != r[0]) | (r[1] != r[1]) | (r[2] != r[2]) | (r[3] != r[3]) | (r[4] != r[4]) | (r[5] != r[5]) | (r[9] != r[9]) |
                         (r[10] != r[10]);
    const bool in_range = r[14] < __builtin_huge_valf();
    const PrefilterArgs pf = make_prefilter_args(EST_RAD1D, thr2, 0.f);
    const float thrp = pf_radial1d_thr(pf.thr);
    for (uint32_t i = 0; i < n; ++i) {
        const double pt[5] = {x[2 * i], x[2 * i + 1], X[3 * i], X[3 * i + 1], X[3 * i + 2]};
        float f[5], w[2];
        pf_radial1d_point(pt, pf.thr, f, w);
        rejected[i] = !(in_range && pf.enabled) ? 0 : (nanflag ? 1 : pf_radial1d_outlier(r, thrp, f, w));
        double r2;
        inlier[i] = radial1d_inlier(rec, pt[0], pt[1], pt[2], pt[3], pt[4], thr2, r2);
    }
    return !(in_range && pf.enabled) ? 2 : (nanflag ? 0 : 1);
}

// Serial evaluation of the LM kernels' algorithm with Refiner<EST_RAD1D>, every sum in correspondence order (k_lm up to 256
// correspondences, k_lm_ordered at every size)
void rd_refine(const double *x, const double *X, uint32_t n, double *pose7, const LMOptions *opt, const uint8_t *mask, uint32_t *iterations,
               double *costs2) {
    using R = Refiner<EST_RAD1D>;
    constexpr int K = R::K, NT = NormalSize<K>::kTotal;
    LMControl ctl;
    ctl.opt = *opt;
    ctl.loss = make_loss(opt->loss_type, opt->loss_scale);
    ctl.done = 0;
    double cur[kParamDoubles] = {0}, trial[kParamDoubles];
    std::memcpy(cur, pose7, sizeof(double) * 7);
    RefineCtx ctx;
    CameraParams cam;
    std::memset(&cam, 0, sizeof(cam));
    double normal[NT], jac_normal[NT], racc = 0;
    uint32_t count = 0;
    auto pass = [&](const double *p, bool jac) {
        R::prepare(p, ctx);
        for (int i = 0; i < NT; ++i)
            normal[i] = 0;
        racc = 0, count = 0;
        for (uint32_t i = 0; i < n; ++i) {
            if (mask && !mask[i])
                continue;
            double r0, r1;
            if (!jac) {
                if (R::residual(p, ctx, cam, x[2 * i], x[2 * i + 1], X[3 * i], X[3 * i + 1], X[3 * i + 2], r0, r1)) {
                    racc += 1.0 * loss_value(ctl.loss, r0 * r0 + r1 * r1);
                    count++;
                }
            } else {
                double J[2 * K];
                if (R::jacobian(p, ctx, cam, x[2 * i], x[2 * i + 1], X[3 * i], X[3 * i + 1], X[3 * i + 2], r0, r1, J))
                    accumulate2<K>(normal, ctl.loss, r0, r1, J, count);
            }
        }
    };
    pass(cur, false);
    lm_begin(ctl, *opt, racc, count);
    costs2[0] = ctl.cost;
    while (!ctl.done) {
        const bool fresh = ctl.rejac != 0;
        if (fresh) {
            pass(cur, true);
            std::memcpy(jac_normal, normal, sizeof(normal));
        }
        lm_solve<K>(ctl, jac_normal, fresh, count);
        if (ctl.done)
            break;
        R::step(cur, ctx, ctl.sol, trial);
        pass(trial, false);
        if (lm_update<K>(ctl, jac_normal, racc, count))
            std::memcpy(cur, trial, sizeof(cur));
    }
    std::memcpy(pose7, cur, sizeof(double) * 7);
    *iterations = ctl.iterations;
    costs2[1] = ctl.cost;
}
}
