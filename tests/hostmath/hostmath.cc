// TEST-ONLY host compilation of the product's device math (poselib_amd/csrc/pl_*.h).
//
// This library exists so that the exact source that hipcc compiles into the gfx950 kernels can be
// exercised on CPU (no GPU in the development container) and compared against the oracle before
// GPU minutes are spent.  It is NOT a CPU fallback: nothing in poselib_amd/ loads it, the C-ABI
// (include/poselib_amd.h) has no code path into it, and the product fails loudly without a GPU.
// Built by tests/hostmath/Makefile with g++ -ffp-contract=off.
#include "../../poselib_amd/csrc/pl_focal.h"
#include "../../poselib_amd/csrc/pl_prefilter.h"
#include "../../poselib_amd/csrc/pl_refine.h"
#include "../../poselib_amd/csrc/pl_refine_cam.h"
#include "../../poselib_amd/csrc/pl_sampler.h"
#include "../../poselib_amd/csrc/pl_sfocal.h"
#include "../../poselib_amd/csrc/pl_score.h"
#include "../../poselib_amd/csrc/pl_solver_h4.h"
#include "../../poselib_amd/csrc/pl_solver_p35pf.h"
#include "../../poselib_amd/csrc/pl_solver_6ptf.h"
#include "../../poselib_amd/csrc/pl_solver_p3p.h"
#include "../../poselib_amd/csrc/pl_solver_rel.h"
#include "../../poselib_amd/csrc/pl_svd3.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace pl;

namespace {

template <int EST> int solve_records(const double *in, double *rec) {
    constexpr int K = EST == EST_ABS ? 3 : EST == EST_REL ? 5 : EST == EST_FUND ? 7 : 4;
    Vec3 a[K], b[K];
    for (int k = 0; k < K; ++k) {
        a[k] = v3(in[3 * k], in[3 * k + 1], in[3 * k + 2]);
        b[k] = v3(in[3 * (K + k)], in[3 * (K + k) + 1], in[3 * (K + k) + 2]);
    }
    if constexpr (EST == EST_ABS) {
        P3PSolution sol[4];
        const int n = p3p(a[0], a[1], a[2], b[0], b[1], b[2], sol);
        for (int m = 0; m < n; ++m)
            store_pose_model(rec + m * kModelStride, sol[m].R, sol[m].t, false);
        return n;
    } else if constexpr (EST == EST_HOM) {
        Mat3 H;
        const int n = homography_4pt(a, b, H, true);
        if (n)
            store_matrix_model(rec, H);
        return n;
    } else if constexpr (EST == EST_FUND) {
        return relpose_7pt_records(a, b, rec, false);
    } else {
        return relpose_5pt_records(a, b, rec);
    }
}

// Serial evaluation of the LM kernel's algorithm (same PL_HD pieces, no block reductions).
template <int EST>
void lm_serial(const double *const *pa, uint32_t n, double *params, const LMOptions &opt, const CameraParams &cam,
               double point_scale, double prefilter_thr2, const uint8_t *mask_in, uint32_t *iterations,
               uint32_t *skipped) {
    using R = Refiner<EST>;
    constexpr int K = R::K;
    constexpr int NT = NormalSize<K>::kTotal;
    LMControl ctl;
    ctl.opt = opt;
    ctl.loss = make_loss(opt.loss_type, opt.loss_scale);
    ctl.done = 0;
    double cur[kParamDoubles], trial[kParamDoubles];
    std::memcpy(cur, params, sizeof(cur));
    std::vector<uint8_t> pre;
    const uint8_t *mask = mask_in;
    *skipped = 0;
    if constexpr (EST == EST_REL) {
        if (prefilter_thr2 > 0) {
            double M[kModelStride];
            Quat q;
            q.w = cur[0], q.x = cur[1], q.y = cur[2], q.z = cur[3];
            store_pose_model_q(M, q, v3(cur[4], cur[5], cur[6]), true);
            pre.resize(n);
            uint32_t c = 0;
            for (uint32_t i = 0; i < n; ++i) {
                double r2;
                pre[i] = sampson_pose_inlier(M, pa[0][i], pa[1][i], pa[2][i], pa[3][i], prefilter_thr2, r2);
                c += pre[i];
            }
            if (c <= 5) {
                *skipped = 1;
                *iterations = 0;
                return;
            }
            mask = pre.data();
        }
    }
    RefineCtx ctx;
    double normal[NT];
    double racc = 0;
    uint32_t count = 0;
    auto pass = [&](const double *p, bool jac) {
        R::prepare(p, ctx);
        for (int i = 0; i < NT; ++i)
            normal[i] = 0;
        racc = 0;
        count = 0;
        for (uint32_t i = 0; i < n; ++i) {
            if (mask && !mask[i])
                continue;
            if constexpr (EST == EST_ABS) {
                const double x = pa[0][i] * point_scale, y = pa[1][i] * point_scale;
                double r0, r1;
                if (!jac) {
                    if (R::residual(p, ctx, cam, x, y, pa[2][i], pa[3][i], pa[4][i], r0, r1)) {
                        racc += 1.0 * loss_value(ctl.loss, r0 * r0 + r1 * r1);
                        count++;
                    }
                } else {
                    double J[2 * K];
                    if (R::jacobian(p, ctx, cam, x, y, pa[2][i], pa[3][i], pa[4][i], r0, r1, J))
                        accumulate2<K>(normal, ctl.loss, r0, r1, J, count);
                }
            } else if constexpr (EST == EST_HOM) {
                double f0, f1, g0, g1;
                if (!jac) {
                    R::residual(ctx, pa[0][i], pa[1][i], pa[2][i], pa[3][i], f0, f1, g0, g1);
                    racc += 1.0 * loss_value(ctl.loss, f0 * f0 + f1 * f1);
                    racc += 1.0 * loss_value(ctl.loss, g0 * g0 + g1 * g1);
                    count += 2;
                } else {
                    double Jf[2 * K], Jb[2 * K];
                    R::jacobian(ctx, pa[0][i], pa[1][i], pa[2][i], pa[3][i], f0, f1, Jf, g0, g1, Jb);
                    accumulate2<K>(normal, ctl.loss, f0, f1, Jf, count);
                    accumulate2<K>(normal, ctl.loss, g0, g1, Jb, count);
                }
            } else {
                if (!jac) {
                    const double r = R::residual(ctx, pa[0][i], pa[1][i], pa[2][i], pa[3][i]);
                    racc += 1.0 * loss_value(ctl.loss, r * r);
                    count++;
                } else {
                    double J[K];
                    const double r = R::jacobian(ctx, pa[0][i], pa[1][i], pa[2][i], pa[3][i], J);
                    accumulate1<K>(normal, ctl.loss, r, J, count);
                }
            }
        }
    };
    double jac_normal[NT];
    pass(cur, false);
    lm_begin(ctl, opt, racc, count);
    while (!ctl.done) {
        const bool fresh = ctl.rejac != 0;
        if (fresh) {
            if constexpr (EST == EST_REL)
                R::prepare_params(cur);
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
    std::memcpy(params, cur, sizeof(cur));
    *iterations = ctl.iterations;
}

} // namespace

extern "C" {

uint32_t hm_draw_samples(uint64_t seed, uint64_t N, int K, uint32_t n_iters, uint32_t *idx, uint32_t *positions) {
    uint64_t pos = 0;
    for (uint32_t i = 0; i < n_iters; ++i) {
        positions[i] = (uint32_t)pos;
        uint32_t used = 0;
        switch (K) {
        case 3:
            used = draw_sample<3>(seed, pos, N, idx + (size_t)i * K);
            break;
        case 4:
            used = draw_sample<4>(seed, pos, N, idx + (size_t)i * K);
            break;
        case 5:
            used = draw_sample<5>(seed, pos, N, idx + (size_t)i * K);
            break;
        case 7:
            used = draw_sample<7>(seed, pos, N, idx + (size_t)i * K);
            break;
        }
        pos += used;
    }
    return (uint32_t)pos;
}

// est: 0 abs (in = 3 bearings + 3 points), 1 rel (5+5 bearings), 2 fund (7+7), 3 hom (4+4)
int hm_solve(int est, const double *in, double *records) {
    switch (est) {
    case EST_ABS:
        return solve_records<EST_ABS>(in, records);
    case EST_REL:
        return solve_records<EST_REL>(in, records);
    case EST_FUND:
        return solve_records<EST_FUND>(in, records);
    default:
        return solve_records<EST_HOM>(in, records);
    }
}

int hm_essential_5pt(const double *in, double *E /* 10 x 9 row-major */) {
    Vec3 a[5], b[5];
    for (int k = 0; k < 5; ++k) {
        a[k] = v3(in[3 * k], in[3 * k + 1], in[3 * k + 2]);
        b[k] = v3(in[3 * (5 + k)], in[3 * (5 + k) + 1], in[3 * (5 + k) + 2]);
    }
    Mat3 Em[10];
    const int n = essential_5pt(a, b, Em);
    for (int i = 0; i < n; ++i)
        std::memcpy(E + 9 * i, Em[i].m, sizeof(double) * 9);
    return n;
}

// P3.5Pf (pl_solver_p35pf.h: the serial statement of the solver whose steps the kernels of focal.hip distribute)
int hm_p35pf(const double *x /* 4 x 2 */, const double *X /* 4 x 3 */, uint32_t /*stride*/, double *poses7, double *focals) {
    Vec3 Xs[4];
    for (int i = 0; i < 4; ++i)
        Xs[i] = v3(X[3 * i], X[3 * i + 1], X[3 * i + 2]);
    P35Solution sol[10];
    const int n = p35pf(x, Xs, sol);
    for (int i = 0; i < n; ++i) {
        const double o[7] = {sol[i].q.w, sol[i].q.x, sol[i].q.y, sol[i].q.z, sol[i].t.x, sol[i].t.y, sol[i].t.z};
        std::memcpy(poses7 + 7 * i, o, sizeof(o));
        focals[i] = sol[i].focal;
    }
    return n;
}
// the 6-point shared-focal solver (pl_solver_6ptf.h: the serial statement)
int hm_relpose_6pt_shared_focal(const double *b1 /* 6 x 3 unit bearings */, const double *b2, uint32_t /*stride*/, double *poses7,
                                double *focals) {
    Vec3 a[6], b[6];
    for (int i = 0; i < 6; ++i) {
        a[i] = v3(b1[3 * i], b1[3 * i + 1], b1[3 * i + 2]);
        b[i] = v3(b2[3 * i], b2[3 * i + 1], b2[3 * i + 2]);
    }
    int n = 0;
    relpose_6pt_shared_focal(a, b, [&](Quat q, Vec3 t, double f) {
        const double o[7] = {q.w, q.x, q.y, q.z, t.x, t.y, t.z};
        std::memcpy(poses7 + 7 * n, o, sizeof(o));
        focals[n++] = f;
    });
    return n;
}
int hm_sturm10(const double *coef, double *roots) { return sturm_roots_deg10(coef, roots); }
int hm_sturm10_flat(const double *coef, double *roots) { // the batched generator's isolation (sturm_isolate_flat)
    SturmWorkLocal w;
    return sturm_roots_deg10_flat(coef, roots, w);
}
// the degree-10 determinant polynomial of a 5-point sample ([x1 5 x 3][x2 5 x 3] unit bearings): what k_rel_roots isolates
void hm_rel5_poly(const double *in, double *c /* 11 */) {
    Vec3 a[5], b[5];
    for (int k = 0; k < 5; ++k) {
        a[k] = v3(in[3 * k], in[3 * k + 1], in[3 * k + 2]);
        b[k] = v3(in[3 * (5 + k)], in[3 * (5 + k) + 1], in[3 * (5 + k) + 2]);
    }
    double nb[36], Az[3][13];
    rel5_front(a, b, nb, Az);
    rel5_poly(Az, c);
}
// The flat isolation with the list capacities of the batched generator (SturmWorkFlat of gen_rel.hip keeps the same two lists in
// LDS) against the recursion-shaped sturm_roots_deg10, on `count` polynomials of 11 coefficients.  Returns how many differ in the
// number, the order or the bits of their roots (*first_bad: the first of them); *max_pending / *max_leaves: the most entries the
// two lists ever held, refused ones included.
namespace {
struct SturmWorkGeneratorCaps : SturmWorkLocal {
    static constexpr int kPendCap = kSturmFlatPendCap, kLeafCap = kSturmFlatLeafCap;
};
struct SturmWorkWatch : SturmWorkLocal { // room for everything: how long do the lists get?
    int max_pending = 0, max_leaves = 0;
    void pend_push(int i, double a, double b, unsigned info) { SturmWorkLocal::pend_push(i, a, b, info), max_pending = std::max(max_pending, i + 1); }
    void uleaf_set(int i, double a, double b) { SturmWorkLocal::uleaf_set(i, a, b), max_leaves = std::max(max_leaves, i + 1); }
};
} // namespace
uint64_t hm_sturm10_flat_generator_caps(const double *coefs, uint64_t count, int64_t *first_bad, int32_t *max_pending, int32_t *max_leaves) {
    static_assert(SturmWorkGeneratorCaps::kPendCap == 6 && SturmWorkGeneratorCaps::kLeafCap == 12, "the generator's capacities");
    uint64_t bad = 0;
    *first_bad = -1, *max_pending = *max_leaves = 0;
    for (uint64_t i = 0; i < count; ++i) {
        const double *c = coefs + 11 * i;
        double want[10], got[10];
        SturmWorkGeneratorCaps w;
        const int nw = sturm_roots_deg10(c, want), ng = sturm_roots_deg10_flat(c, got, w);
        if (nw != ng || std::memcmp(want, got, sizeof(double) * nw) != 0) {
            if (!bad)
                *first_bad = (int64_t)i;
            ++bad;
        }
        SturmWorkWatch watch;
        double tmp[10];
        sturm_roots_deg10_flat(c, tmp, watch);
        *max_pending = std::max(*max_pending, watch.max_pending);
        *max_leaves = std::max(*max_leaves, watch.max_leaves);
    }
    return bad;
}

// Build a model record from (q,t) or a row-major 3x3, as the generate kernel stores it.
void hm_pose_record(const double *q4, const double *t3, int essential, double *rec) {
    Quat q;
    q.w = q4[0], q.x = q4[1], q.y = q4[2], q.z = q4[3];
    store_pose_model_q(rec, q, v3(t3[0], t3[1], t3[2]), essential != 0);
}

// Score one model record against SoA points; per-point r2 / inlier flags are returned for bit-exact
// comparison with the oracle.  score follows k_finalize: sum_inl r2 + (N - cnt) thr2 (serial sum).
double hm_score(int est, const double *rec, const double *const *pa, uint32_t n, double thr2, uint32_t *count,
                uint8_t *flags, double *r2_out) {
    uint32_t c = 0;
    double s = 0;
    for (uint32_t i = 0; i < n; ++i) {
        double r2 = 0;
        bool in;
        switch (est) {
        case EST_ABS:
            in = reproj_inlier(rec, pa[0][i], pa[1][i], pa[2][i], pa[3][i], pa[4][i], thr2, r2);
            break;
        case EST_REL:
            in = sampson_pose_inlier(rec, pa[0][i], pa[1][i], pa[2][i], pa[3][i], thr2, r2);
            break;
        case EST_FUND:
            in = sampson_inlier(rec, pa[0][i], pa[1][i], pa[2][i], pa[3][i], thr2, r2);
            break;
        default:
            in = homography_inlier(rec, pa[0][i], pa[1][i], pa[2][i], pa[3][i], thr2, r2);
        }
        if (flags)
            flags[i] = in;
        if (r2_out)
            r2_out[i] = r2;
        // the reference's summation orders (robust/utils.cc): the reprojection score adds the inliers' r^2 and the
        // outliers' share in one product at the end (:57-63); the two-view scores add r^2 OR thr^2 correspondence by
        // correspondence (:188-198, 230-235, 320-325) - k_score_seq does the same on the device
        if (in) {
            c++;
            s += r2;
        } else if (est != EST_ABS) {
            s += thr2;
        }
    }
    *count = c;
    return est == EST_ABS ? s + (double)(n - c) * thr2 : s;
}

void hm_matrix_record(const double *M9, double *rec) {
    Mat3 M;
    for (int i = 0; i < 9; ++i)
        M.m[i] = M9[i];
    store_matrix_model(rec, M);
}

// The scoring kernels' conservative fp32 pre-filter, operation for operation (kernels.hip k_score_stream pass A):
// out[i] = 1 when correspondence i is PROVEN not to be an inlier of the model.  Returns 0 when the filter is
// disabled for these parameters (every point is then evaluated exactly).
int hm_prefilter(int est, const double *rec, const double *const *pa, uint32_t n, double thr2, float xy_absmax,
                 uint8_t *out) {
    const PrefilterArgs pf = make_prefilter_args(est, thr2, xy_absmax);
    const float *r = reinterpret_cast<const float *>(rec + kShadowOff);
    std::memset(out, 0, n);
    if (!pf.enabled)
        return 0;
    uint32_t flag;
    std::memcpy(&flag, &r[13], 4);
    if (flag != 0u) { // NaN model: no inliers at all
        std::memset(out, 1, n);
        return 1;
    }
    for (uint32_t i = 0; i < n; ++i) {
        if (est == EST_ABS) {
            const float fw = pf_point_abs(pa[2][i], pa[3][i], pa[4][i], pf.gx);
            const float gt = pf_up(pf.gx * r[12]);
            out[i] = pf_abs_outlier(r, gt, pf.thr, (float)pa[0][i], (float)pa[1][i], (float)pa[2][i], (float)pa[3][i],
                                    (float)pa[4][i], fw);
        } else {
            float nanb, nsq, nanb_thr;
            pf_point_two_view(pa[0][i], pa[1][i], pa[2][i], pa[3][i], pf.thr, nanb, nsq, nanb_thr);
            const float a0 = (float)pa[0][i], a1 = (float)pa[1][i], b0 = (float)pa[2][i], b1 = (float)pa[3][i];
            if (est == EST_HOM)
                out[i] = pf_hom_outlier(r, (32.f * kPfU) * r[14], pf.thr, a0, a1, b0, b1, nanb_thr);
            else
                out[i] = pf_sampson_outlier(r, (16.f * kPfU) * r[14], pf.t1, a0, a1, b0, b1, pf_point_sampson_w(nanb, nsq, pf));
        }
    }
    return 1;
}

// The Sampson pre-filter in its fp16 / matrix-core form (k_score_mfma2; pl_prefilter.h): the same operand builders as the
// kernels, the two forms accumulated in fp32 in k-slot order.  Returns 0 when that form is not available for these
// parameters (coordinates beyond 8, threshold out of range).  random_order != 0: the products are accumulated in a
// pseudo-random order instead (the bound must hold for any order the matrix pipe may use).
int hm_prefilter16(int est, const double *rec, const double *const *pa, uint32_t n, double thr2, float uv_absmax,
                   uint32_t random_order, uint8_t *out) {
    const PrefilterArgs pf = make_prefilter_args(est, thr2, uv_absmax);
    std::memset(out, 0, n);
    if (!pf.enabled || !(pf.t16 > 0.f) || (est != EST_REL && est != EST_FUND))
        return 0;
    const float *r = reinterpret_cast<const float *>(rec + kShadowOff);
    uint32_t flag;
    std::memcpy(&flag, &r[13], 4);
    Sampson16Operand m;
    pf16_sampson_model(rec + kMatOff, flag != 0u, m);
    uint64_t rng = 0x9e3779b97f4a7c15ull * (random_order + 1);
    for (uint32_t i = 0; i < n; ++i) {
        Sampson16Operand p;
        pf16_sampson_point(pa[0][i], pa[1][i], pa[2][i], pa[3][i], true, pf.t16, p);
        if (!random_order) {
            out[i] = pf16_sampson_outlier(m, p, pf.t16);
            continue;
        }
        int oc[32], os[16];
        for (int k = 0; k < 32; ++k)
            oc[k] = k;
        for (int k = 0; k < 16; ++k)
            os[k] = k;
        auto next = [&]() {
            rng ^= rng << 13, rng ^= rng >> 7, rng ^= rng << 17;
            return (uint32_t)(rng >> 33);
        };
        for (int k = 31; k > 0; --k)
            std::swap(oc[k], oc[next() % (k + 1)]);
        for (int k = 15; k > 0; --k)
            std::swap(os[k], os[next() % (k + 1)]);
        float Cc = 0.f, S = 0.f;
        for (int k = 0; k < 32; ++k)
            Cc = fmaf(pf_half_to_float(m.c[oc[k]]), pf_half_to_float(p.c[oc[k]]), Cc);
        for (int k = 0; k < 16; ++k)
            S = fmaf(pf_half_to_float(m.s[os[k]]), pf_half_to_float(p.s[os[k]]), S);
        const float d = fmaf(pf.t16, S, -(Cc * Cc));
        uint32_t bits;
        std::memcpy(&bits, &d, 4);
        out[i] = (uint8_t)(bits >> 31);
    }
    return 1;
}

// The reprojection pre-filter in its fp16 / matrix-core form (k_shadow16 + k_score_mfma; pl_prefilter.h): the same operand
// builders as the kernels, the four half-plane forms accumulated in fp32 in k-slot order or (random_order != 0) in a
// pseudo-random order.  Returns 0 when that form is not available (threshold above 1, coordinates out of range).
int hm_prefilter16_abs(const double *rec, const double *const *pa, uint32_t n, double thr2, float xy_absmax,
                       uint32_t random_order, uint8_t *out) {
    const PrefilterArgs pf = make_prefilter_args(EST_ABS, thr2, xy_absmax);
    std::memset(out, 0, n);
    if (!pf.enabled || !(pf.g16 > 0.f) || !(pf.thr <= 1.0f))
        return 0;
    Abs16Model m;
    pf16_abs_model(reinterpret_cast<const float *>(rec + kShadowOff), pf.c16, pf.thr, m);
    uint64_t rng = 0x9e3779b97f4a7c15ull * (random_order + 1);
    for (uint32_t i = 0; i < n; ++i) {
        Abs16Point p;
        pf16_abs_point(pa[0][i], pa[1][i], pa[2][i], pa[3][i], pa[4][i], true, pf.g16, pf.thr, p);
        int order[16];
        for (int k = 0; k < 16; ++k)
            order[k] = k;
        if (random_order)
            for (int k = 15; k > 0; --k) {
                rng ^= rng << 13, rng ^= rng >> 7, rng ^= rng << 17;
                std::swap(order[k], order[(rng >> 33) % (uint64_t)(k + 1)]);
            }
        out[i] = pf16_abs_outlier(m, p, random_order ? order : nullptr);
    }
    return 1;
}

// The homography pre-filter in its fp16 / matrix-core form (k_hom16 + k_score_mfmah; pl_prefilter.h): the same operand
// builders as the kernels, the four linear forms accumulated in fp32 in k-slot order or (random_order != 0) in a
// pseudo-random order.  Returns 0 when that form is not available (coordinates beyond 8, threshold out of range).
int hm_prefilter16_hom(const double *rec, const double *const *pa, uint32_t n, double thr2, float uv_absmax,
                       uint32_t random_order, uint8_t *out) {
    const PrefilterArgs pf = make_prefilter_args(EST_HOM, thr2, uv_absmax);
    std::memset(out, 0, n);
    if (!pf.enabled || !(pf.h16 > 0.f))
        return 0;
    const float *r = reinterpret_cast<const float *>(rec + kShadowOff);
    uint32_t flag;
    std::memcpy(&flag, &r[13], 4);
    Hom16Model m;
    pf16_hom_model(rec + kMatOff, flag != 0u, pf.h16, m);
    uint64_t rng = 0x9e3779b97f4a7c15ull * (random_order + 1);
    for (uint32_t i = 0; i < n; ++i) {
        Hom16Point p;
        pf16_hom_point(pa[0][i], pa[1][i], pa[2][i], pa[3][i], true, pf.h16, p);
        int order[32];
        for (int k = 0; k < 32; ++k)
            order[k] = k;
        if (random_order)
            for (int k = 31; k > 0; --k) {
                rng ^= rng << 13, rng ^= rng >> 7, rng ^= rng << 17;
                std::swap(order[k], order[(rng >> 33) % (uint64_t)(k + 1)]);
            }
        out[i] = pf16_hom_outlier(m, p, random_order ? order : nullptr);
    }
    return 1;
}

// the device form of the Nielsen update's cube (pl_refine.h lm_cube_fma), for the comparison with glibc's pow(x, 3)
void hm_lm_cube(const double *x, uint64_t n, double *out) {
    for (uint64_t i = 0; i < n; ++i)
        out[i] = lm_cube_fma(x[i]);
}

// fp16 conversions of pl_prefilter.h (checked against numpy's float16 by the tests)
void hm_half_rn(const float *v, uint64_t n, uint16_t *bits, float *back) {
    for (uint64_t i = 0; i < n; ++i) {
        bits[i] = pf_half_rn(v[i]);
        back[i] = pf_half_to_float(bits[i]);
    }
}

void hm_mask_abs(const double *rec, const double *const *pa, uint32_t n, double thr2, uint8_t *mask) {
    for (uint32_t i = 0; i < n; ++i)
        mask[i] = reproj_mask(rec, pa[0][i], pa[1][i], pa[2][i], pa[3][i], pa[4][i], thr2);
}

void hm_unproject(const CameraParams *cam, const double *xp, uint32_t n, double *out) {
    for (uint32_t i = 0; i < n; ++i)
        camera_unproject(*cam, xp[2 * i], xp[2 * i + 1], out[2 * i], out[2 * i + 1]);
}

void hm_lm(int est, const double *const *pa, uint32_t n, double *params, const LMOptions *opt, const CameraParams *cam,
           double point_scale, double prefilter_thr2, const uint8_t *mask, uint32_t *iterations, uint32_t *skipped) {
    switch (est) {
    case EST_ABS:
        lm_serial<EST_ABS>(pa, n, params, *opt, *cam, point_scale, prefilter_thr2, mask, iterations, skipped);
        break;
    case EST_REL:
        lm_serial<EST_REL>(pa, n, params, *opt, *cam, point_scale, prefilter_thr2, mask, iterations, skipped);
        break;
    case EST_FUND:
        lm_serial<EST_FUND>(pa, n, params, *opt, *cam, point_scale, prefilter_thr2, mask, iterations, skipped);
        break;
    default:
        lm_serial<EST_HOM>(pa, n, params, *opt, *cam, point_scale, prefilter_thr2, mask, iterations, skipped);
    }
}

// hm_lm with the Nielsen update's cube in the device's form (lm_cube_fma instead of pow) when device_cube != 0: the serial CPU
// model of k_lm_ordered, bit for bit (PL_LM_CUBE_HOST_SWITCH, defined by this build alone)
void hm_lm_ex(int est, const double *const *pa, uint32_t n, double *params, const LMOptions *opt, const CameraParams *cam,
              double point_scale, double prefilter_thr2, const uint8_t *mask, int device_cube, uint32_t *iterations, uint32_t *skipped) {
    lm_cube_host_switch().device_form = device_cube != 0;
    lm_cube_host_switch().calls = 0;
    hm_lm(est, pa, n, params, opt, cam, point_scale, prefilter_thr2, mask, iterations, skipped);
    lm_cube_host_switch().device_form = 0;
}
// the arguments of the Nielsen update's cube in the last hm_lm_ex run (the first 256 of them): returns how many were written
uint32_t hm_lm_cube_args(double *out, uint32_t capacity) {
    const LMCubeHostSwitch &s = lm_cube_host_switch();
    const uint32_t n = std::min<uint32_t>(std::min<uint32_t>(s.calls, 256u), capacity);
    for (uint32_t i = 0; i < n; ++i)
        out[i] = s.args[i];
    return n;
}

// The parameter block with which a fundamental matrix (row-major) enters the LM kernels: the driver's own factorisation
// (pl_svd3.h fundamental_lm_params, what driver.cc lm_params_from_record calls)
void hm_fund_params(const double *F9, double *params) {
    Mat3 F;
    std::memcpy(F.m, F9, sizeof(F.m));
    for (int i = 0; i < kParamDoubles; ++i)
        params[i] = 0.0;
    fundamental_lm_params(F, params);
}
// lm_cube of pl_refine.h as this build compiles it (PL_LM_CUBE_HOST_SWITCH): the device's form when device_cube != 0, pow otherwise
double hm_lm_cube_switched(double x, int device_cube) {
    lm_cube_host_switch().device_form = device_cube != 0;
    lm_cube_host_switch().calls = 0;
    const double r = lm_cube(x);
    lm_cube_host_switch().device_form = 0;
    return r;
}

// Serial evaluation of k_lm_cam's algorithm (lm_cam.hip): the same rows, the same per-entry sums in correspondence order.
// Returns 1, with nothing touched, when the flags select no parameter of the model (M = 0: the driver sends such a bundle to k_lm,
// and lm_solve_k has no K = 6), 0 otherwise.
int hm_lm_cam(const double *const *pa, uint32_t n, double *params, const LMOptions *opt, CameraParams *cam_io, int cam_flags,
              double point_scale, const uint8_t *mask, uint32_t *iterations, double *costs /* initial, final, invalid steps */) {
    {
        int none[kCamMaxParams];
        if (camera_refinement_idx(cam_io->model_id, cam_flags, none) == 0)
            return 1;
    }
    LMControl ctl;
    ctl.opt = *opt;
    ctl.loss = make_loss(opt->loss_type, opt->loss_scale);
    ctl.done = 0;
    double cur[kParamDoubles], trial[kParamDoubles];
    std::memcpy(cur, params, sizeof(cur));
    CameraParams cam_cur = *cam_io, cam_trial = *cam_io;
    int idx[kCamMaxParams];
    const int M = camera_refinement_idx(cam_cur.model_id, cam_flags, idx);
    const int K = 6 + M, NT = K * (K + 1) / 2 + K;
    double normal[kCamMaxEntries], racc = 0;
    uint32_t count = 0;
    double R[9];
    auto rotation_of = [&](const double *p) {
        Quat q;
        q.w = p[0], q.x = p[1], q.y = p[2], q.z = p[3];
        const Mat3 Rm = quat_to_rotmat(q);
        for (int i = 0; i < 9; ++i)
            R[i] = Rm.m[i];
    };
    auto cost_pass = [&](const double *p, const CameraParams &cam) {
        rotation_of(p);
        racc = 0, count = 0;
        for (uint32_t i = 0; i < n; ++i) {
            double term;
            if (mask && !mask[i])
                continue;
            if (abs_cam_cost(p, R, cam, ctl.loss, pa[0][i] * point_scale, pa[1][i] * point_scale, pa[2][i], pa[3][i], pa[4][i], term))
                racc += term, count++;
        }
    };
    auto jacobian_pass = [&](const double *p, const CameraParams &cam) {
        rotation_of(p);
        for (int e = 0; e < NT; ++e)
            normal[e] = 0;
        count = 0;
        for (uint32_t i = 0; i < n; ++i) {
            double row[kCamRow];
            if (mask && !mask[i])
                continue;
            if (!abs_cam_row(p, R, cam, ctl.loss, pa[0][i] * point_scale, pa[1][i] * point_scale, pa[2][i], pa[3][i], pa[4][i], row))
                continue;
            for (int e = 0; e < NT; ++e)
                normal[e] += cam_entry_term(row, cam_entry_of(e, K, idx));
            count++;
        }
    };
    cost_pass(cur, cam_cur);
    lm_begin(ctl, *opt, racc, count);
    while (!ctl.done) {
        const bool fresh = ctl.rejac != 0;
        if (fresh)
            jacobian_pass(cur, cam_cur);
        lm_solve_k(K, ctl, normal, fresh, count);
        if (ctl.done)
            break;
        abs_cam_step(cur, cam_cur, ctl.sol, idx, M, trial, cam_trial);
        cost_pass(trial, cam_trial);
        if (lm_update_k(K, ctl, normal, racc, count)) {
            std::memcpy(cur, trial, sizeof(cur));
            cam_cur = cam_trial;
        }
    }
    std::memcpy(params, cur, sizeof(cur));
    *cam_io = cam_cur;
    *iterations = ctl.iterations;
    costs[0] = ctl.initial_cost, costs[1] = ctl.cost;
    costs[2] = (double)ctl.invalid_steps;
    return 0;
}
// hm_lm_cam with the Nielsen update's cube in the device's form when device_cube != 0 (as hm_lm_ex): the serial model of k_lm_cam,
// bit for bit; hm_lm_cube_args holds the cube's arguments afterwards
int hm_lm_cam_ex(const double *const *pa, uint32_t n, double *params, const LMOptions *opt, CameraParams *cam_io, int cam_flags,
                 double point_scale, const uint8_t *mask, int device_cube, uint32_t *iterations, double *costs) {
    lm_cube_host_switch().device_form = device_cube != 0;
    lm_cube_host_switch().calls = 0;
    const int r = hm_lm_cam(pa, n, params, opt, cam_io, cam_flags, point_scale, mask, iterations, costs);
    lm_cube_host_switch().device_form = 0;
    return r;
}

// The shared-focal refiner as k_sfocal_lm runs it (sfocal.hip): every sum correspondence after correspondence.  prefilter_thr2 > 0:
// refine_model of the estimator (relative_pose.cc:173-203) - the correspondences with Sampson error below it, nothing when <= 6.
// Returns 1 when the refinement was skipped.
int hm_sfocal_lm(const double *const *pa, uint32_t n, double *pose7, double *focal, const LMOptions *opt, double prefilter_thr2,
                 const uint8_t *mask_in, uint32_t *iterations, double *costs /* initial, final, invalid steps */) {
    std::vector<uint8_t> keep(n, 1);
    if (prefilter_thr2 > 0) {
        FocalModel m;
        std::memcpy(m.q, pose7, sizeof(double) * 4);
        std::memcpy(m.t, pose7 + 4, sizeof(double) * 3);
        m.f = *focal;
        double F[9];
        sfocal_F_score(m, F);
        uint32_t cnt = 0;
        for (uint32_t i = 0; i < n; ++i) {
            keep[i] = sampson_sq(F, pa[0][i], pa[1][i], pa[2][i], pa[3][i]) < prefilter_thr2;
            cnt += keep[i];
        }
        if (cnt <= 6)
            return 1;
    } else if (mask_in) {
        for (uint32_t i = 0; i < n; ++i)
            keep[i] = mask_in[i] != 0;
    }
    LMControl ctl;
    ctl.opt = *opt;
    ctl.loss = make_loss(opt->loss_type, opt->loss_scale);
    ctl.done = 0;
    double cur[kParamDoubles] = {0}, trial[kParamDoubles];
    std::memcpy(cur, pose7, sizeof(double) * 7);
    cur[kSFocalFocalSlot] = *focal;
    double normal[kSFocalEntries], racc = 0;
    uint32_t count = 0;
    SFocalCtx ctx;
    auto cost_pass = [&](const double *p) {
        sfocal_prepare(p, ctx, false);
        racc = 0, count = 0;
        for (uint32_t i = 0; i < n; ++i) {
            if (!keep[i])
                continue;
            const double r = sfocal_residual(ctx, pa[0][i], pa[1][i], pa[2][i], pa[3][i]);
            racc += 1.0 * loss_value(ctl.loss, r * r);
            count++;
        }
    };
    auto jacobian_pass = [&](double *p) {
        Refiner<EST_REL>::prepare_params(p);
        sfocal_prepare(p, ctx, true);
        for (int e = 0; e < kSFocalEntries; ++e)
            normal[e] = 0;
        count = 0;
        for (uint32_t i = 0; i < n; ++i) {
            double row[kSFocalRow];
            if (!keep[i] || !sfocal_row(ctx, ctl.loss, pa[0][i], pa[1][i], pa[2][i], pa[3][i], row))
                continue;
            for (int e = 0; e < kSFocalEntries; ++e)
                normal[e] += sfocal_entry_term(row, e);
            count++;
        }
    };
    cost_pass(cur);
    lm_begin(ctl, *opt, racc, count);
    while (!ctl.done) {
        const bool fresh = ctl.rejac != 0;
        if (fresh)
            jacobian_pass(cur);
        lm_solve<6>(ctl, normal, fresh, count);
        if (ctl.done)
            break;
        sfocal_step(cur, ctl.sol, trial);
        cost_pass(trial);
        if (lm_update<6>(ctl, normal, racc, count))
            std::memcpy(cur, trial, sizeof(cur));
    }
    std::memcpy(pose7, cur, sizeof(double) * 7);
    *focal = cur[kSFocalFocalSlot];
    *iterations = ctl.iterations;
    costs[0] = ctl.initial_cost, costs[1] = ctl.cost;
    costs[2] = (double)ctl.invalid_steps;
    return 0;
}
// hm_sfocal_lm with the device's cube when device_cube != 0 (as hm_lm_ex): the serial model of k_sfocal_lm, bit for bit
int hm_sfocal_lm_ex(const double *const *pa, uint32_t n, double *pose7, double *focal, const LMOptions *opt, double prefilter_thr2,
                    const uint8_t *mask_in, int device_cube, uint32_t *iterations, double *costs) {
    lm_cube_host_switch().device_form = device_cube != 0;
    lm_cube_host_switch().calls = 0;
    const int r = hm_sfocal_lm(pa, n, pose7, focal, opt, prefilter_thr2, mask_in, iterations, costs);
    lm_cube_host_switch().device_form = 0;
    return r;
}

void hm_factorized_F(const double *params, double *F) { factorized_F(params, F); }

// The argument streams of the libm tests.  tests/test_libm_vs_glibc.py walks them here against the host's libm;
// tests/test_gpu_device_math.py reads the same arguments through hm_math_args and sends them to the device.
namespace {
enum { GEN_CBRT = 0, GEN_ACOS = 1, GEN_COS = 2, GEN_SIN = 3, GEN_SINCOS = 4 };
struct ArgStream {
    int which, mode; // mode: cbrt only - 0 any bit pattern; 1 uniform in [-10, 10]; 2 log-uniform magnitudes 2^-60..2^60,
                     // both signs; 3 subnormals
    uint64_t s, i = 0;
    ArgStream(int which_, int mode_, uint64_t seed) : which(which_), mode(mode_), s(seed * 0x9E3779B97F4A7C15ull + 88172645463325252ull) {}
    uint64_t rnd() {
        s ^= s << 13, s ^= s >> 7, s ^= s << 17;
        return s;
    }
    double next() {
        static const uint64_t edges[] = {0x3fc00000, 0x3fd00000, 0x3fe00000, 0x3fe80000, 0x3fed8000, 0x3fee8000, 0x3fef0000, 0x3ff00000};
        double x;
        if (which == GEN_CBRT) {
            const uint64_t r = rnd();
            if (mode == 0) {
                std::memcpy(&x, &r, 8);
            } else if (mode == 1) {
                x = ((double)(r >> 11) / 9007199254740992.0 - 0.5) * 20.0;
            } else if (mode == 2) {
                x = std::ldexp((double)(r >> 11) / 9007199254740992.0 + 0.5, (int)(rnd() % 121) - 60);
                if (r & 1)
                    x = -x;
            } else {
                const uint64_t b = r & 0x800fffffffffffffull;
                std::memcpy(&x, &b, 8);
            }
        } else if (which == GEN_SINCOS) { // [-6, 6], [0, 0.9], [-2.4, 2.4] and down to 2^-40
            const double u = (double)(rnd() >> 11) / 9007199254740992.0;
            x = (i % 4 == 0) ? (u * 12 - 6) : (i % 4 == 1) ? u * 0.9 : (i % 4 == 2) ? (u * 4.8 - 2.4) : std::ldexp(2 * u - 1, -(int)((s >> 3) % 40));
        } else {
            const double u = (double)(rnd() >> 11) / 9007199254740992.0;
            if (which == GEN_ACOS) { // (-1, 1) incl. the neighbourhoods of +-1 and 0 and the interval edges of the piecewise expansion
                switch (i % 5) {
                case 0:
                    x = 2 * u - 1;
                    break;
                case 1:
                    x = (u < 0.5 ? -1 : 1) * (1 - std::ldexp(u, -(int)(rnd() % 40)));
                    break;
                case 2:
                    x = std::ldexp(2 * u - 1, -(int)(rnd() % 60));
                    break;
                case 3:
                    x = (0.96875 + u * 0.03125) * ((rnd() & 1) ? 1 : -1);
                    break;
                default: {
                    uint64_t b = edges[rnd() % 8] << 32;
                    b += (int64_t)(rnd() % 2000) - 1000;
                    std::memcpy(&x, &b, 8);
                    if (rnd() & 1)
                        x = -x;
                }
                }
            } else if (which == GEN_COS) { // [-6, 6], [0, 1.0472] and tiny arguments
                x = (i % 3 == 0) ? (u * 12 - 6) : (i % 3 == 1) ? u * 1.0472 : std::ldexp(2 * u - 1, -(int)(rnd() % 40));
            } else { // sin: [-2.4, 2.4], [0, 0.5] and tiny arguments
                x = (i % 3 == 0) ? (u * 4.8 - 2.4) : (i % 3 == 1) ? u * 0.5 : std::ldexp(2 * u - 1, -(int)(rnd() % 40));
            }
        }
        ++i;
        return x;
    }
};

// The host's libm, one function per loop and per (non-inlined) function: at -O1 and above GCC merges sin and cos of the same
// argument into one sincos() call, whose last bit differs (pl_libm.h pl_sincos).
__attribute__((noinline)) void glibc_cbrt(const double *x, uint64_t n, double *out) {
    for (uint64_t i = 0; i < n; ++i)
        out[i] = std::cbrt(x[i]);
}
__attribute__((noinline)) void glibc_acos(const double *x, uint64_t n, double *out) {
    for (uint64_t i = 0; i < n; ++i)
        out[i] = std::acos(x[i]);
}
__attribute__((noinline)) void glibc_cos(const double *x, uint64_t n, double *out) {
    for (uint64_t i = 0; i < n; ++i)
        out[i] = std::cos(x[i]);
}
__attribute__((noinline)) void glibc_sin(const double *x, uint64_t n, double *out) {
    for (uint64_t i = 0; i < n; ++i)
        out[i] = std::sin(x[i]);
}
__attribute__((noinline)) void glibc_sincos(const double *x, uint64_t n, double *sn, double *cs) {
    for (uint64_t i = 0; i < n; ++i)
        sincos(x[i], &sn[i], &cs[i]);
}
__attribute__((noinline)) void glibc_pow3(const double *x, uint64_t n, double *out) {
    volatile double three = 3.0; // (a literal exponent would let the compiler expand the call)
    for (uint64_t i = 0; i < n; ++i)
        out[i] = std::pow(x[i], (double)three);
}
} // namespace

// `count` arguments of stream `which` (GEN_*), written to out
void hm_math_args(int which, int mode, uint64_t seed, uint64_t count, double *out) {
    ArgStream g(which, mode, seed);
    for (uint64_t i = 0; i < count; ++i)
        out[i] = g.next();
}

// glibc on n arguments: which = GEN_CBRT .. GEN_SIN as above, GEN_SINCOS (out[0, n): sine, out[n, 2n): cosine), 5: pow(x, 3)
void hm_glibc(int which, const double *x, uint64_t n, double *out) {
    switch (which) {
    case GEN_CBRT:
        glibc_cbrt(x, n, out);
        break;
    case GEN_ACOS:
        glibc_acos(x, n, out);
        break;
    case GEN_COS:
        glibc_cos(x, n, out);
        break;
    case GEN_SIN:
        glibc_sin(x, n, out);
        break;
    case GEN_SINCOS:
        glibc_sincos(x, n, out, out + n);
        break;
    default:
        glibc_pow3(x, n, out);
    }
}

// pl_libm.h against the host's libm (glibc): number of arguments on which pl_cbrt and cbrt differ in any bit (modes: ArgStream)
uint64_t hm_cbrt_mismatches(uint64_t count, uint64_t seed, int mode, double *first_bad) {
    ArgStream g(GEN_CBRT, mode, seed);
    uint64_t bad = 0;
    for (uint64_t i = 0; i < count; ++i) {
        const double x = g.next();
        const double mine = pl_cbrt(x), host = std::cbrt(x);
        if (std::memcmp(&mine, &host, 8) != 0 && !(mine != mine && host != host)) {
            if (!bad && first_bad)
                *first_bad = x;
            ++bad;
        }
    }
    return bad;
}
double hm_cbrt(double x) { return pl_cbrt(x); }
double hm_sin(double x) { return pl_sin(x); }
double hm_cos(double x) { return pl_cos(x); }
// pl_sincos against the host's sincos(): number of arguments (GEN_SINCOS) on which either result differs in any bit
uint64_t hm_sincos_mismatches(uint64_t count, uint64_t seed, double *first_bad) {
    ArgStream g(GEN_SINCOS, 0, seed);
    uint64_t bad = 0;
    for (uint64_t i = 0; i < count; ++i) {
        const double x = g.next();
        double a, b, c, d;
        pl_sincos(x, a, b);
        sincos(x, &c, &d);
        if (std::memcmp(&a, &c, 8) != 0 || std::memcmp(&b, &d, 8) != 0) {
            if (!bad && first_bad)
                *first_bad = x;
            ++bad;
        }
    }
    return bad;
}

// pl_log1p against the host's log1p: the number of arguments on which they differ in any bit.  A quarter of the arguments each:
// u 2^e with e = -30 .. 29 (what r2 / scale^2 of a Cauchy loss can be), -u (down to -1), any bit pattern (NaN, inf, subnormals,
// arguments below -1), and the neighbourhoods of the routine's branch points (sqrt(2) - 1, sqrt(2) / 2 - 1, 2^-29, 2^-54, 2^53)
uint64_t hm_log1p_mismatches(uint64_t count, uint64_t seed, double *first_bad) {
    uint64_t s = seed * 0x9e3779b97f4a7c15ull + 0x2545f4914f6cdd1dull, bad = 0;
    auto rnd = [&]() {
        s ^= s << 13, s ^= s >> 7, s ^= s << 17;
        return s;
    };
    const double edges[6] = {0.41421356237309503, -0.29289321881345248, 0x1p-29, 0x1p-54, 0x1p53, -1.0};
    for (uint64_t i = 0; i < count; ++i) {
        const double u = (double)(rnd() >> 11) / 9007199254740992.0;
        const uint64_t r = rnd();
        double x;
        switch (i % 4) {
        case 0: x = std::ldexp(u, (int)(r % 60) - 30); break;
        case 1: x = -u; break;
        case 2: std::memcpy(&x, &r, 8); break;
        default: x = edges[r % 6] * (1.0 + (2 * u - 1) * std::ldexp(1.0, -(int)((r >> 8) % 53))); break;
        }
        const double got = pl_log1p(x), want = std::log1p(x);
        if (std::memcmp(&got, &want, 8) != 0 && !(got != got && want != want)) {
            if (bad == 0 && first_bad)
                *first_bad = x;
            ++bad;
        }
    }
    return bad;
}

// which: 0 acos (GEN_ACOS), 1 cos (GEN_COS), 2 sin (GEN_SIN): arguments on which pl_libm.h and the host's libm differ in any bit
uint64_t hm_libm_mismatches(int which, uint64_t count, uint64_t seed, double *first_bad) {
    ArgStream g(GEN_ACOS + which, 0, seed);
    uint64_t bad = 0;
    for (uint64_t i = 0; i < count; ++i) {
        const double x = g.next();
        double mine, host;
        if (which == 0)
            mine = pl_acos(x), host = std::acos(x);
        else if (which == 1)
            mine = pl_cos(x), host = std::cos(x);
        else
            mine = pl_sin(x), host = std::sin(x);
        if (std::memcmp(&mine, &host, 8) != 0 && !(mine != mine && host != host)) {
            if (!bad && first_bad)
                *first_bad = x;
            ++bad;
        }
    }
    return bad;
}

} // extern "C"

// ---- ransac_pnpf: the product's loop (pl_focal.h focal_lo_ransac) over a back end that evaluates the device functions serially -
// the generator's and the scorer's per-lane code, hm_lm_cam for the local optimisation.  What this checks on the CPU: the
// decisions of the loop against the oracle's ransac_pnpf; what it cannot check: the kernels' indexing and memory traffic. ----
namespace {
struct HostFocalBackend {
    const double *const *pa;
    uint32_t n;
    uint64_t seed;
    double thr2, max_error, max_focal;

    void score_one(const FocalModel &m, uint32_t &count, double &sum) const {
        double R[9];
        focal_rotation(m, R);
        count = 0, sum = 0.0;
        for (uint32_t i = 0; i < n; ++i) {
            double r2;
            if (focal_reproj_inlier(R, m.t, m.f, pa[0][i], pa[1][i], pa[2][i], pa[3][i], pa[4][i], thr2, r2))
                count++, sum += r2;
        }
    }
    int minimal(uint64_t pos_base, const uint32_t *positions, uint32_t B, std::vector<FocalModel> &models,
                std::vector<uint32_t> &num_models, std::vector<uint32_t> &counts, std::vector<double> &sums, const uint32_t *samples = nullptr) {
        models.clear(), counts.clear(), sums.clear(); // (compact: one entry per model, in (iteration, slot) order)
        num_models.assign(B, 0);
        for (uint32_t it = 0; it < B; ++it) {
            uint32_t idx[kFocalSample];
            if (samples)
                for (int k = 0; k < kFocalSample; ++k)
                    idx[k] = samples[(size_t)it * kFocalSample + k];
            else
                draw_sample<kFocalSample>(seed, pos_base + positions[it], n, idx);
            double xs[8];
            Vec3 X[4];
            for (int k = 0; k < 4; ++k) {
                xs[2 * k] = pa[0][idx[k]], xs[2 * k + 1] = pa[1][idx[k]];
                X[k] = v3(pa[2][idx[k]], pa[3][idx[k]], pa[4][idx[k]]);
            }
            P35Solution sol[kFocalMaxModels];
            const int ns = p35pf(xs, X, sol);
            uint32_t m = 0;
            for (int i = 0; i < ns; ++i) {
                if (sol[i].focal < 0 || (max_focal >= 0 && sol[i].focal > max_focal))
                    continue;
                FocalModel o;
                o.q[0] = sol[i].q.w, o.q[1] = sol[i].q.x, o.q[2] = sol[i].q.y, o.q[3] = sol[i].q.z;
                o.t[0] = sol[i].t.x, o.t[1] = sol[i].t.y, o.t[2] = sol[i].t.z;
                o.f = sol[i].focal;
                uint32_t cnt = 0;
                double sum = 0.0;
                score_one(o, cnt, sum);
                models.push_back(o), counts.push_back(cnt), sums.push_back(sum);
                ++m;
            }
            num_models[it] = m;
        }
        return 0;
    }
    int score(const std::vector<FocalModel> &models, std::vector<uint32_t> &counts, std::vector<double> &sums) {
        counts.assign(models.size(), 0);
        sums.assign(models.size(), 0.0);
        for (size_t i = 0; i < models.size(); ++i)
            score_one(models[i], counts[i], sums[i]);
        return 0;
    }
    int refine_score(const std::vector<FocalModel> &seeds, std::vector<FocalModel> &refined, std::vector<uint32_t> &counts,
                     std::vector<double> &sums) {
        int rc = refine(seeds, refined);
        return rc ? rc : score(refined, counts, sums);
    }
    int refine(const std::vector<FocalModel> &seeds, std::vector<FocalModel> &refined) {
        refined = seeds;
        LMOptions lo;
        lo.max_iterations = 25, lo.loss_type = LOSS_TRUNCATED, lo.lambda_update = 0, lo.damping = 0;
        lo.loss_scale = max_error, lo.gradient_tol = 1e-12, lo.step_tol = 1e-8, lo.relative_cost_tol = 1e-10;
        lo.initial_lambda = 1e-3, lo.min_lambda = 1e-10, lo.max_lambda = 1e10, lo.lambda_factor = 10.0;
        for (FocalModel &m : refined) {
            double params[kParamDoubles] = {0};
            for (int i = 0; i < 4; ++i)
                params[i] = m.q[i];
            for (int i = 0; i < 3; ++i)
                params[4 + i] = m.t[i];
            CameraParams cam;
            std::memset(&cam, 0, sizeof(cam));
            cam.model_id = CAM_SIMPLE_PINHOLE, cam.num_params = 3, cam.p[0] = m.f;
            uint32_t its;
            double costs[3];
            hm_lm_cam(pa, n, params, &lo, &cam, CAM_REFINE_FOCAL, 1.0, nullptr, &its, costs);
            for (int i = 0; i < 4; ++i)
                m.q[i] = params[i];
            for (int i = 0; i < 3; ++i)
                m.t[i] = params[4 + i];
            m.f = cam.p[0];
        }
        return 0;
    }
};
} // namespace

// PROSAC for the two focal-length loops below (sampling.cc:85-136): process-wide switch of the test build
static int g_hm_prosac = 0;
static uint64_t g_hm_max_prosac = 100000;
extern "C" void hm_set_prosac(int on, uint64_t max_prosac_iterations) { g_hm_prosac = on, g_hm_max_prosac = max_prosac_iterations; }

extern "C" void hm_ransac_pnpf(const double *const *pa, uint32_t n, uint64_t max_iterations, uint64_t min_iterations, uint64_t seed,
                               double dyn_mult, double success_prob, int score_initial, double max_error, double min_fov, double *pose7,
                               double *focal, uint8_t *mask, uint64_t *stats5 /* refinements, iterations, num_inliers, hypotheses, evaluated */,
                               double *model_score) {
    FocalLoopOptions o;
    o.max_iterations = max_iterations, o.min_iterations = min_iterations, o.seed = seed;
    o.dyn_num_trials_mult = dyn_mult, o.success_prob = success_prob, o.score_initial_model = score_initial != 0;
    o.progressive_sampling = g_hm_prosac != 0, o.max_prosac_iterations = g_hm_max_prosac;
    o.max_error = max_error;
    o.max_focal = focal_max_focal_length(pa[0], pa[1], n, min_fov);
    HostFocalBackend be{pa, n, seed, max_error * max_error, max_error, o.max_focal};
    FocalModel best;
    std::memset(&best, 0, sizeof(best));
    best.q[0] = 1.0, best.f = 1.0;
    FocalLoopStats st;
    focal_lo_ransac(be, n, o, &best, &st);
    std::memcpy(pose7, best.q, sizeof(double) * 4);
    std::memcpy(pose7 + 4, best.t, sizeof(double) * 3);
    *focal = best.f;
    double R[9];
    focal_rotation(best, R);
    for (uint32_t i = 0; i < n; ++i)
        mask[i] = focal_reproj_mask(R, best.t, best.f, pa[0][i], pa[1][i], pa[2][i], pa[3][i], pa[4][i], max_error * max_error) ? 1 : 0;
    stats5[0] = st.refinements, stats5[1] = st.iterations, stats5[2] = st.num_inliers, stats5[3] = st.hypotheses, stats5[4] = st.iterations_evaluated;
    *model_score = st.model_score;
}

// ---- ransac_shared_focal_relpose: pl_focal.h's loop template with SharedFocalTraits over a serial evaluation of the device
// functions (6-point generator, in-order MSAC score, hm_sfocal_lm) ----
namespace {
struct HostSFocalBackend {
    const double *const *pa;
    uint32_t n;
    uint64_t seed;
    double thr2, max_error;

    void score_one(const FocalModel &m, uint32_t &count, double &score) const {
        double F[9];
        sfocal_F_score(m, F);
        count = 0, score = 0.0;
        for (uint32_t i = 0; i < n; ++i) {
            const double r2 = sampson_sq(F, pa[0][i], pa[1][i], pa[2][i], pa[3][i]);
            if (r2 < thr2)
                count++, score += r2;
            else
                score += thr2;
        }
    }
    int minimal(uint64_t pos_base, const uint32_t *positions, uint32_t B, std::vector<FocalModel> &models,
                std::vector<uint32_t> &num_models, std::vector<uint32_t> &counts, std::vector<double> &sums, const uint32_t *samples = nullptr) {
        models.clear(), counts.clear(), sums.clear(); // (compact: one entry per model, in (iteration, slot) order)
        num_models.assign(B, 0);
        for (uint32_t it = 0; it < B; ++it) {
            uint32_t idx[kSFocalSample];
            if (samples)
                for (int k = 0; k < kSFocalSample; ++k)
                    idx[k] = samples[(size_t)it * kSFocalSample + k];
            else
                draw_sample<kSFocalSample>(seed, pos_base + positions[it], n, idx);
            Vec3 a[6], b[6];
            for (int k = 0; k < 6; ++k) {
                a[k] = bearing(pa[0][idx[k]], pa[1][idx[k]]);
                b[k] = bearing(pa[2][idx[k]], pa[3][idx[k]]);
            }
            uint32_t m = 0;
            relpose_6pt_shared_focal(a, b, [&](Quat q, Vec3 t, double f) {
                FocalModel o;
                o.q[0] = q.w, o.q[1] = q.x, o.q[2] = q.y, o.q[3] = q.z;
                o.t[0] = t.x, o.t[1] = t.y, o.t[2] = t.z;
                o.f = f;
                uint32_t cnt = 0;
                double sum = 0.0;
                score_one(o, cnt, sum);
                models.push_back(o), counts.push_back(cnt), sums.push_back(sum);
                ++m;
            });
            num_models[it] = m;
        }
        return 0;
    }
    int score(const std::vector<FocalModel> &models, std::vector<uint32_t> &counts, std::vector<double> &sums) {
        counts.assign(models.size(), 0);
        sums.assign(models.size(), 0.0);
        for (size_t i = 0; i < models.size(); ++i)
            score_one(models[i], counts[i], sums[i]);
        return 0;
    }
    int refine_score(const std::vector<FocalModel> &seeds, std::vector<FocalModel> &refined, std::vector<uint32_t> &counts,
                     std::vector<double> &sums) {
        int rc = refine(seeds, refined);
        return rc ? rc : score(refined, counts, sums);
    }
    int refine(const std::vector<FocalModel> &seeds, std::vector<FocalModel> &refined) {
        refined = seeds;
        LMOptions lo;
        lo.max_iterations = 25, lo.loss_type = LOSS_TRUNCATED, lo.lambda_update = 0, lo.damping = 0;
        lo.loss_scale = max_error, lo.gradient_tol = 1e-12, lo.step_tol = 1e-8, lo.relative_cost_tol = 1e-10;
        lo.initial_lambda = 1e-3, lo.min_lambda = 1e-10, lo.max_lambda = 1e10, lo.lambda_factor = 10.0;
        for (FocalModel &m : refined) {
            uint32_t its;
            double costs[3];
            hm_sfocal_lm(pa, n, m.q, &m.f, &lo, 5 * thr2, nullptr, &its, costs); // (q and t are adjacent: 7 doubles)
        }
        return 0;
    }
};
} // namespace

extern "C" void hm_ransac_shared_focal(const double *const *pa, uint32_t n, uint64_t max_iterations, uint64_t min_iterations,
                                       uint64_t seed, double dyn_mult, double success_prob, int score_initial, double max_error,
                                       double *pose7, double *focal, uint8_t *mask,
                                       uint64_t *stats5 /* refinements, iterations, num_inliers, hypotheses, evaluated */,
                                       double *model_score) {
    FocalLoopOptions o;
    o.max_iterations = max_iterations, o.min_iterations = min_iterations, o.seed = seed;
    o.dyn_num_trials_mult = dyn_mult, o.success_prob = success_prob, o.score_initial_model = score_initial != 0;
    o.progressive_sampling = g_hm_prosac != 0, o.max_prosac_iterations = g_hm_max_prosac;
    o.max_error = max_error;
    o.max_focal = -1.0;
    HostSFocalBackend be{pa, n, seed, max_error * max_error, max_error};
    FocalModel best;
    std::memcpy(best.q, pose7, sizeof(double) * 4);
    std::memcpy(best.t, pose7 + 4, sizeof(double) * 3);
    best.f = *focal;
    if (!score_initial) {
        std::memset(&best, 0, sizeof(best));
        best.q[0] = 1.0, best.f = 1.0;
    }
    FocalLoopStats st;
    focal_lo_ransac_t<SharedFocalTraits>(be, n, o, &best, &st);
    std::memcpy(pose7, best.q, sizeof(double) * 4);
    std::memcpy(pose7 + 4, best.t, sizeof(double) * 3);
    *focal = best.f;
    double F[9];
    sfocal_F_score(best, F);
    for (uint32_t i = 0; i < n; ++i)
        mask[i] = sampson_sq(F, pa[0][i], pa[1][i], pa[2][i], pa[3][i]) < max_error * max_error ? 1 : 0;
    stats5[0] = st.refinements, stats5[1] = st.iterations, stats5[2] = st.num_inliers, stats5[3] = st.hypotheses, stats5[4] = st.iterations_evaluated;
    *model_score = st.model_score;
}

// The product's host-side SVD at the entry of the fundamental-matrix refinement (pl_svd3.h), row-major in and out.
// ---- pl_general_eigenvalues (pl_solver_p35pf.h: Hessenberg + Francis QR, the eigenvalue routine of the P3.5Pf action matrix) on
// matrices given explicitly: real and imaginary parts in the routine's order
extern "C" int hm_general_eigenvalues(int n, const double *mats, int count, double *wr_out, double *wi_out) {
    if (n != 10)
        return -1;
    for (int k = 0; k < count; ++k) {
        double a[100];
        for (int e = 0; e < 100; ++e)
            a[e] = mats[(size_t)k * 100 + e];
        pl_general_eigenvalues<10, double *>(a, wr_out + (size_t)k * 10, wi_out + (size_t)k * 10);
    }
    return 0;
}
// sturm_n_roots<15> (pl_sturm_n.h) and danilevsky_charpoly<15> (pl_action_template.h)
extern "C" int hm_sturm15(const double *coef16, double tol, double *roots) { return sturm_n_roots<15>(coef16, roots, tol); }
extern "C" void hm_charpoly15(const double *A225, double *p16) {
    double a[225];
    std::memcpy(a, A225, sizeof(a));
    danilevsky_charpoly<15>(a, p16);
}
extern "C" void hm_svd3(const double *A9, double *U9, double *s3, double *V9) {
    Mat3 A, U, V;
    std::memcpy(A.m, A9, sizeof(A.m));
    svd3(A, U, s3, V);
    std::memcpy(U9, U.m, sizeof(U.m));
    std::memcpy(V9, V.m, sizeof(V.m));
}
