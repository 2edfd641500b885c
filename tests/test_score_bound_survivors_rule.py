"""Stage S of the bound tier on the CPU: in front of the fp32 verdict every pre-selected position behind the
lead is judged on the matrix-core filter's SURVIVOR count over all N correspondences - c_ub = the survivors, an upper bound of the
inliers since the filter drops proven outliers only, and s_lb = (N - c_ub) thr^2, since every proven outlier shares thr^2 exactly
and every other pair at least 0: the tier's rule with these two, which is the exact pruning rule at S = N with 0 for the sum.

Flagship scenes 1, 2, 3, 4 x LEAD oracle models each, survivors from the host build of the filter's fp16 form
(test_score_count_rule.flagship_survivors), bounds from the host build of the tier's per-pair functions (hostmath_bound):
  1. stage S drops no position that the records rule lists;
  2. the three-stage tier (S, verdict, residuals) keeps every candidate and leaves at most what the two-stage tier leaves;
  3. stage S leaves at most half of the pre-selected positions behind the lead - the condition for the stage to pay: the fp32
     verdict (90 vector instructions per entry and chunk) then runs on half the entries or fewer.  (The host models give 53 / 134,
     57 / 138 and 64 / 162.)"""
import functools

import numpy as np
import pytest

import hostmath_bound_lib as HB
import hostmath_lib as HM
import prune_cases as PC
import test_score_bound_rule as BR
import test_score_count_rule as CR

THR2 = PC.THR ** 2
SEEDS = (1, 2, 3)


def stage_s_bounds(surv, N, thr2=THR2):
    """(c_ub, s_lb) of stage S per position: the survivors over all N, and thr^2 for each of the other pairs - rounded down as
    the device's product of thr^2 and an integer number of pairs is (one ulp below the nearest is not above the exact one)"""
    c_ub = surv.sum(axis=1).astype(np.int64)
    return c_ub, (N - c_ub) * thr2 * (1.0 - 2.0 ** -52)


@functools.lru_cache(maxsize=None)
def flagship(seed):
    """the scene's reference, survivor flags and prune model, the pre-selection, and per stage the flags of what the tier leaves
    with and without stage S in front - computed once, read by every test of this file"""
    H = 4 * PC.LEAD
    r2, inl, surv, live, cp = CR.flagship_survivors(seed, H)
    N = inl.shape[1]
    m = PC.prune_model(r2, inl, live, THR2, cp)
    assert m["cstar"] < m["chunks"]
    sel = CR.preselect(surv, live, THR2, cp, m["lead_max"], m["lead_min"], m["cstar"], m["chunks"])
    behind = live & (np.cumsum(live) > PC.LEAD)
    tier = functools.partial(BR.bound_tier, live=live, lead_max=m["lead_max"], lead_min=m["lead_min"], cstar=m["cstar"], chunks=m["chunks"])
    c_s, s_s = stage_s_bounds(surv, N)
    assert (c_s >= m["full_counts"])[live].all() and (s_s <= m["full_scores"])[live].all(), "stage S's bounds are on the wrong side"
    after_s = tier(c_s, s_s, sel) & sel
    # the fp32 stages on the same scene and models as flagship_survivors builds
    cols, _, x, X = BR.scene_cols(seed)
    sc = PC.Scene.__new__(PC.Scene)
    sc.a, sc.b = np.ascontiguousarray(x), np.ascontiguousarray(X)
    models = sc.p3p_models(len(x), H, 300 + seed)
    xy = float(np.abs(x).max())

    @functools.lru_cache(maxsize=None)
    def bound(k, residual):
        en, L, maybe, quanta = HB.bound(HM.pose_record(models[k][:4], models[k][4:]), cols, THR2, xy, residual)
        assert en and not (inl[k] & ~maybe).any()
        return int(maybe.sum()), THR2 * (float(quanta.astype(np.int64).sum()) / BR.HM_SCALE) * (1.0 - 2.0 ** -52)

    def fp32_stages(keep):
        c_ub = np.zeros(H, dtype=np.int64)
        s_lb = np.zeros(H)
        for residual in (False, True):
            for k in np.flatnonzero(keep & behind):
                c_ub[k], s_lb[k] = bound(int(k), residual)
                assert c_ub[k] >= m["full_counts"][k] and s_lb[k] <= m["full_scores"][k]
            keep = tier(c_ub, s_lb, keep) & keep
        return keep

    return {"m": m, "sel": sel, "behind": behind, "after_s": after_s, "two": fp32_stages(sel.copy()), "three": fp32_stages(after_s.copy()),
            "want": PC.records_rule(m["full_counts"], m["full_scores"])}


@pytest.mark.parametrize("seed", SEEDS)
def test_stage_s_drops_no_candidate(seed):
    f = flagship(seed)
    assert len(f["want"]) > 0 and f["after_s"][f["want"]].all(), (seed, "stage S dropped a listed candidate")
    assert not (f["after_s"] & ~f["sel"]).any()


@pytest.mark.parametrize("seed", SEEDS)
def test_three_stages_keep_every_candidate_and_leave_no_more_than_two(seed):
    f = flagship(seed)
    assert f["three"][f["want"]].all(), (seed, "the three-stage tier dropped a listed candidate")
    two, three = int((f["two"] & f["behind"]).sum()), int((f["three"] & f["behind"]).sum())
    print(f"seed {seed}: pre-selected behind the lead {int((f['sel'] & f['behind']).sum())}, two stages leave {two}, three leave {three}")
    assert three <= two
    assert not (f["three"] & ~f["two"]).any(), (seed, "an entry the verdict and the residuals drop survives behind stage S")


@pytest.mark.parametrize("seed", SEEDS)
def test_stage_s_leaves_at_most_half(seed):
    f = flagship(seed)
    pre, left = int((f["sel"] & f["behind"]).sum()), int((f["after_s"] & f["behind"]).sum())
    print(f"seed {seed}: stage S leaves {left} of {pre} pre-selected positions behind the lead")
    assert pre > 0 and 2 * left <= pre
