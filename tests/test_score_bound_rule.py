"""The bound tier of the pruned scorer on the CPU: between pre-selection and exact scores every pre-selected
position behind the lead gets an fp32 upper bound c_ub of its inlier count and a lower bound s_lb of its score, and is dropped iff
c_ub <= lead_max and s_lb > lead_min (1 + margin).

1. Property: pf_abs_verdict_lower and pf_abs_r2_lower (pl_prefilter.h, host build tests/hostmath_bound) against hostmath's fp64 residuals and inlier flags.
   A pair's share of the MSAC score is r^2 for an inlier and thr^2 for everything else (a point behind the camera included, whatever
   its r^2); for every pair min(L, thr^2) and the quantum both stay at or below that share, and "may be an inlier" is set wherever
   the reference has an inlier.
2. Rule, in numpy, on the lists of tests/test_gpu_score_prune.py: bounds = the exact values degraded by random admissible slack; the
   tier drops nothing that the records rule lists and changes no candidate list.
3. Flagship condition, seeds 1, 2, 3, 4 x LEAD models, the host build of the real bounds - the verdict stage, then the residual
   stage on what it leaves: at most a tenth of the pre-selected positions behind the lead survive the tier."""
import numpy as np
import pytest

import hostmath_bound_lib as HB
import hostmath_lib as HM
import prune_cases as PC
import test_gpu_score_prune as TP
import test_score_count_rule as CR
from poselib_amd import synth
from prune_cases import GROUP, SINGLE

THR2 = PC.THR ** 2


# ---- 1. the per-pair bound ------------------------------------------------------------------------------------------------------------
def check_pairs(tag, q, t, cols, thr2=THR2):
    """one model against correspondences cols = (x, y, X, Y, Z); returns (pairs, inliers, pairs with a positive bound)"""
    cols = [np.ascontiguousarray(c, dtype=np.float64) for c in cols]
    rec = HM.pose_record(q, t)
    _, _, inl, r2 = HM.score("abs", rec, cols, thr2)
    with np.errstate(invalid="ignore"):
        xy = float(np.nanmax(np.abs(np.r_[cols[0], cols[1]])))
    share = np.where(inl, r2, thr2)
    en, L, maybe, quanta = HB.bound(rec, cols, thr2, xy, residual=False)  # the first stage's verdict: +inf or 0
    if not en:
        return 0, 0, 0
    assert (np.isinf(L) | (L == 0)).all() and (quanta[np.isinf(L)] == HB.SCALE).all() and (quanta[L == 0] == 0).all(), tag
    assert not (np.isinf(L) & inl).any() and (maybe == (L == 0)).all(), (tag, "the verdict excludes an inlier")
    en, L, maybe, quanta = HB.bound(rec, cols, thr2, xy)
    assert not np.isnan(L).any(), tag
    bad = np.flatnonzero(~(np.minimum(L.astype(np.float64), thr2) <= share))
    assert len(bad) == 0, (tag, "min(L, thr^2) above the pair's share", bad[:5], L[bad[:5]], share[bad[:5]])
    bad = np.flatnonzero(~(quanta.astype(np.float64) * (thr2 / HB.SCALE) <= share))
    assert len(bad) == 0, (tag, "quantum above the pair's share", bad[:5], quanta[bad[:5]], share[bad[:5]])
    assert (quanta <= HB.SCALE).all(), tag
    bad = np.flatnonzero(inl & ~maybe)
    assert len(bad) == 0, (tag, "an inlier without the flag", bad[:5], L[bad[:5]], r2[bad[:5]])
    return len(L), int(inl.sum()), int((L > 0).sum())


def scene_cols(seed, n=5000, ratio=0.7):
    d = synth.absolute_pose_scene(n, ratio, seed)
    x = (np.asarray(d["p2d"]) - 500.0) / PC.FOCAL
    X = np.asarray(d["p3d"], float)
    gt = np.r_[np.asarray(d["q_gt"], float), np.asarray(d["t_gt"], float)]
    return [x[:, 0], x[:, 1], X[:, 0], X[:, 1], X[:, 2]], gt, x, X


def test_bound_on_flagship_scenes():
    tot = np.zeros(3, dtype=np.int64)
    for seed in (1, 2):
        cols, gt, x, X = scene_cols(seed)
        sc = PC.Scene.__new__(PC.Scene)
        sc.a, sc.b = np.ascontiguousarray(x), np.ascontiguousarray(X)
        models = sc.p3p_models(len(x), 150, 40 + seed)
        models = models[~np.isnan(models).any(axis=1)]
        for k, m in enumerate(list(models) + [gt, PC.perturbed_gt(sc_gt(gt), 1e-4, seed)]):
            tot += check_pairs(("flagship", seed, k), m[:4], m[4:], cols)
    print("pairs, inliers, pairs with a positive bound:", tot)
    assert tot[1] > 1000 and tot[2] > 0.9 * (tot[0] - tot[1])  # the bound says something about the outliers


def sc_gt(gt):
    s = PC.Scene.__new__(PC.Scene)
    s.gt = gt
    return s


def planted(gt, X, radius, rs):
    """2-D points at `radius` (an array) from the exact projections of X under gt, in random directions"""
    R = PC.quat_to_rotmat(gt[:4])
    Z = X @ R.T + gt[4:]
    ang = rs.uniform(0, 2 * np.pi, len(X))
    return Z[:, 0] / Z[:, 2] + radius * np.cos(ang), Z[:, 1] / Z[:, 2] + radius * np.sin(ang), Z


def test_bound_with_residuals_planted_at_the_threshold():
    rs = np.random.RandomState(11)
    cols, gt, x, X = scene_cols(3, 2000, 0.0)
    steps = rs.randint(-8, 9, len(X))
    radius = PC.THR * (1.0 + steps * 2.0 ** -52)  # within a few ulp of the threshold, on both sides
    for scale in (1.0, 1.0 + 2.0 ** -30, 1.0 - 2.0 ** -30, 1.0 + 2.0 ** -20, 1.0 - 2.0 ** -20, 1.0 + 2.0 ** -14, 1.0 - 2.0 ** -14):
        px, py, _ = planted(gt, X, radius * scale, rs)
        n, ninl, _ = check_pairs(("planted", scale), gt[:4], gt[4:], [px, py, X[:, 0], X[:, 1], X[:, 2]])
        print("scale - 1 =", scale - 1.0, "inliers", ninl, "of", n)
        assert (ninl > 0) if scale <= 1.0 else (ninl < n)


def test_bound_with_depths_at_near_and_below_zero():
    rs = np.random.RandomState(12)
    cols, gt, x, X = scene_cols(4, 1500, 0.0)
    R = PC.quat_to_rotmat(gt[:4])
    depths = np.r_[0.0, [s * 10.0 ** e for e in (-300, -30, -12, -9, -7, -6, -5, -4, -3, -2, -1, 0) for s in (1, -1)]]
    for z2 in depths:
        # move every point along the optical axis to depth z2 (up to the rounding of the move itself), keep its image point
        Z = X @ R.T + gt[4:]
        Zn = np.c_[Z[:, 0], Z[:, 1], np.full(len(Z), z2)]
        Xn = (Zn - gt[4:]) @ R
        check_pairs(("depth", z2), gt[:4], gt[4:], [cols[0], cols[1], Xn[:, 0], Xn[:, 1], Xn[:, 2]])
        # and image points that the moved points hit exactly, where that is a finite number
        with np.errstate(divide="ignore", invalid="ignore"):
            hx, hy = Zn[:, 0] / z2, Zn[:, 1] / z2
        ok = np.isfinite(hx) & np.isfinite(hy) & (np.abs(hx) < 1e30) & (np.abs(hy) < 1e30)
        if ok.any():
            check_pairs(("depth hit", z2), gt[:4], gt[4:], [hx[ok], hy[ok], Xn[ok, 0], Xn[ok, 1], Xn[ok, 2]])


def test_bound_beyond_the_filters_range_and_field_of_view():
    rs = np.random.RandomState(13)
    cols, gt, x, X = scene_cols(5, 1000, 0.3)
    # |X| and |t|: up to and beyond fp32, and so small that squares leave the normal range
    for s in (1e3, 1e6, 1e12, 1e20, 1e30, 1e38, 1e39, 1e200, 1e300, 1e-10, 1e-14, 1e-17, 1e-19, 1e-22, 1e-30, 1e-40):
        for sx, st in ((s, 1.0), (1.0, s), (s, s)):
            check_pairs(("range", sx, st), gt[:4], gt[4:] * st, [cols[0], cols[1], X[:, 0] * sx, X[:, 1] * sx, X[:, 2] * sx])
    # a field of view beyond 90 degrees: image coordinates up to 50, hit within a threshold or missed
    R = PC.quat_to_rotmat(gt[:4])
    dirs = np.c_[rs.uniform(-50, 50, 1000), rs.uniform(-50, 50, 1000), np.ones(1000)]
    Z = dirs * rs.uniform(0.05, 20.0, (1000, 1))
    Xw = (Z - gt[4:]) @ R
    for off in (0.0, 0.5 * PC.THR, 0.999 * PC.THR, 1.001 * PC.THR, 3 * PC.THR, 1.0):
        n, ninl, _ = check_pairs(("fov", off), gt[:4], gt[4:], [dirs[:, 0] + off, dirs[:, 1], Xw[:, 0], Xw[:, 1], Xw[:, 2]])
        assert (ninl > 0.9 * n) if off < 0.99 * PC.THR else (ninl < 0.1 * n if off > 1.01 * PC.THR else True), (off, ninl)


def test_bound_with_nan_infinite_and_unnormalised_models():
    cols, gt, x, X = scene_cols(6, 600, 0.3)
    for i in range(7):
        for v in (np.nan, np.inf, -np.inf, 1e39, -1e39, 1e300):
            m = gt.copy()
            m[i] = v
            check_pairs(("model", i, v), m[:4], m[4:], cols)
    for s in (0.5, 0.999, 1.001, 2.0, 1e3):  # (the record's matrix is not a rotation: q is used as given)
        check_pairs(("scaled q", s), gt[:4] * s, gt[4:], cols)
    for v in (np.nan, np.inf):  # ... and correspondences that are not numbers
        c2 = [c.copy() for c in cols]
        c2[0][::7] = v
        c2[3][::5] = v
        check_pairs(("points", v), gt[:4], gt[4:], c2)


# ---- 2. the rule ----------------------------------------------------------------------------------------------------------------------
def bound_tier(c_ub, s_lb, selected, live, lead_max, lead_min, cstar, chunks, margin=PC.MARGIN_SCORE, lead=PC.LEAD):
    """flags of the positions the tier does NOT drop; selected: what the pre-selection kept"""
    in_lead = live & (np.cumsum(live) - 1 < lead)
    dropped = selected & live & ~in_lead & (c_ub <= lead_max) & (s_lb > lead_min * (1.0 + margin))
    if cstar == chunks:
        dropped[:] = False
    return ~dropped


@pytest.mark.parametrize("slack", [0.0, 1e-4, 0.05, 0.5])
def test_the_bound_rule_drops_no_candidate(slack):
    rs = np.random.RandomState(int(1e4 * slack) + 3)
    dropped_total = behind_total = 0
    for ratio, N, H in TP.CASES:
        models, (r2, inl, live) = TP.list_of(ratio, N, H)
        for route in (SINGLE, GROUP):
            for init in ((0, PC.DBL_MAX), (N, 0.0), None):
                cp = PC.chunk_points(N, route)
                free = PC.prune_model(r2, inl, live, THR2, cp)
                if init is None:  # an incumbent between the list's median and its best
                    good = np.sort(free["full_scores"][live])
                    init = (int(np.sort(free["full_counts"][live])[-max(2, live.sum() // 8)]), float(good[max(1, live.sum() // 8)]))
                m = PC.prune_model(r2, inl, live, THR2, cp, *init)
                # admissible bounds: per pair a share in [(1 - slack) share, share], flags = inliers plus some of the others
                share = np.where(inl, r2, THR2) * (1.0 - slack * rs.rand(*inl.shape))
                c_ub = (inl | (rs.rand(*inl.shape) < slack)).sum(axis=1)
                s_lb = np.floor(share / THR2 * HM_SCALE).sum(axis=1) * THR2 / HM_SCALE * (1.0 - 2.0 ** -52)
                sel = CR.preselect(inl, live, THR2, cp, m["lead_max"], m["lead_min"], m["cstar"], m["chunks"])
                keep = bound_tier(c_ub, s_lb, sel, live, m["lead_max"], m["lead_min"], m["cstar"], m["chunks"]) & sel
                want = PC.records_rule(m["full_counts"], m["full_scores"], *init)
                assert keep[want].all(), (ratio, N, H, route, init, "a listed candidate was dropped")
                cnt = np.where(keep, m["full_counts"], 0)
                sco = np.where(keep, m["full_scores"], N * THR2)
                assert PC.records_rule(cnt, sco, *init) == want, (ratio, N, H, route, init)
                behind = live & (np.cumsum(live) > PC.LEAD)
                dropped_total += int((sel & ~keep).sum())
                behind_total += int((sel & behind).sum())
    print(f"slack {slack}: the tier drops {dropped_total} of {behind_total} pre-selected positions behind the leads")


HM_SCALE = float(HB.SCALE)


# ---- 3. the flagship condition ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_flagship_bound_tier_keeps_at_most_a_tenth(seed):
    H = 4 * PC.LEAD
    r2, inl, surv, live, cp = CR.flagship_survivors(seed, H)
    m = PC.prune_model(r2, inl, live, THR2, cp)
    assert m["cstar"] < m["chunks"]
    sel = CR.preselect(surv, live, THR2, cp, m["lead_max"], m["lead_min"], m["cstar"], m["chunks"])
    behind = live & (np.cumsum(live) > PC.LEAD)
    pre = np.flatnonzero(sel & behind)
    # the real bound of the pre-selected positions (the same scene and models as flagship_survivors builds)
    cols, _, x, X = scene_cols(seed)
    sc = PC.Scene.__new__(PC.Scene)
    sc.a, sc.b = np.ascontiguousarray(x), np.ascontiguousarray(X)
    models = sc.p3p_models(len(x), H, 300 + seed)
    xy = float(np.abs(x).max())
    c_ub = np.zeros(H, dtype=np.int64)
    s_lb = np.zeros(H)
    keep = sel.copy()
    left1 = 0
    for residual in (False, True):  # the verdict for all of them, the residual bound for what that leaves
        for k in np.flatnonzero(keep & behind):
            en, L, maybe, quanta = HB.bound(HM.pose_record(models[k][:4], models[k][4:]), cols, THR2, xy, residual)
            assert en and not (inl[k] & ~maybe).any()
            c_ub[k] = maybe.sum()
            s_lb[k] = THR2 * (float(quanta.astype(np.int64).sum()) / HM_SCALE) * (1.0 - 2.0 ** -52)
            assert c_ub[k] >= m["full_counts"][k] and s_lb[k] <= m["full_scores"][k]
        keep = bound_tier(c_ub, s_lb, keep, live, m["lead_max"], m["lead_min"], m["cstar"], m["chunks"]) & keep
        if not residual:
            left1 = int((keep & behind).sum())
    print(f"seed {seed}: the verdict stage leaves {left1} of {len(pre)}")
    left = int((keep & behind).sum())
    want = PC.records_rule(m["full_counts"], m["full_scores"])
    assert keep[want].all()
    print(f"seed {seed}: pre-selected behind the lead {len(pre)}, the bound tier keeps {left}; median inliers of the pre-selected "
          f"{int(np.median(m['full_counts'][pre])) if len(pre) else 0}, lead_max {m['lead_max']}")
    assert len(pre) > 0 and 10 * left <= len(pre)
