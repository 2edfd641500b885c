// TEST-ONLY host build of the bound tier's per-pair functions (pl_prefilter.h: pf_abs_verdict_lower of the first stage, residual = 0,
// and pf_abs_r2_lower of the second, residual = 1, with their helpers), operation for
// operation as k_score_bound evaluates it: slack of the model, slack of the correspondence, L, the "may be an inlier" flag and the
// quantum of min(L, thr^2) / thr^2.  (The device's reciprocal is v_rcp_f32, here an IEEE division: both are inside the rounding
// charge of the derivation.)
#include "../../poselib_amd/csrc/pl_prefilter.h"

#include <cstdint>
#include <cstring>

using namespace pl;

extern "C" {
// rec: a model record as hostmath's hm_pose_record writes it; pa: x, y, X, Y, Z.  Returns 0 when the pre-filter is disabled for these
// parameters (nothing written).  xy_absmax: max(|x|, |y|) over the problem's 2-D points.
int hb_bound(int residual, const double *rec, const double *const *pa, uint32_t n, double thr2, float xy_absmax, float *L_out,
             uint8_t *maybe, uint32_t *quanta) {
    const PrefilterArgs pf = make_prefilter_args(0 /* EST_ABS */, thr2, xy_absmax);
    if (!pf.enabled)
        return 0;
    const float *r = reinterpret_cast<const float *>(rec + kShadowOff);
    const float gt = pf_abs_bound_slack(r, pf.gx);
    for (uint32_t i = 0; i < n; ++i) {
        const float fw = pf_point_abs(pa[2][i], pa[3][i], pa[4][i], pf.gx);
        const float x = (float)pa[0][i], y = (float)pa[1][i], X = (float)pa[2][i], Y = (float)pa[3][i], Z = (float)pa[4][i];
        const float L = residual ? pf_abs_r2_lower(r, gt, x, y, X, Y, Z, fw) : pf_abs_verdict_lower(r, gt, pf.thr, x, y, X, Y, Z, fw);
        L_out[i] = L;
        maybe[i] = L < pf.thr2_up ? 1 : 0;
        quanta[i] = pf_bound_quantum(L, pf.inv_thr2_dn);
    }
    return 1;
}
}
