"""The pre-selection of the two-tier pruned scorer on the CPU: a position behind the lead is dropped on its SURVIVOR count cs' of the
chunks [0, c*) - what the matrix-core filter lets through, a superset of the inliers - iff cs' + (N - S) <= lead_max and
(S - cs') thr^2 > lead_min (1 + margin): the exact rule of tests/prune_cases.py with cs' for cs and 0 for the sum.

1. Whatever the survivor sets are, as long as they contain the inliers, the pre-selection drops only what prune_model prunes: every
   list of tests/test_gpu_score_prune.py, survivors = the reference's inliers plus random non-inliers at several rates.
2. On the flagship scenes (5000 correspondences, 70 % outliers), with the host build of the filter's fp16 form as the survivor
   source, the pre-selection keeps at most twice what the exact rule keeps - the condition for the second tier to stay small."""
import numpy as np
import pytest

import hostmath_lib as HM
import prune_cases as PC
import test_gpu_score_prune as TP
from poselib_amd import synth
from prune_cases import GROUP, SINGLE


def preselect(surv, live, thr2, chunk_points, lead_max, lead_min, cstar, chunks, margin=PC.MARGIN_SCORE, lead=PC.LEAD):
    """surv: (H, N) survivor flags.  Returns the (H,) flags of the positions the count rule does NOT drop."""
    H, N = surv.shape
    pos = np.cumsum(live) - 1
    in_lead = live & (pos < lead)
    S = min(cstar * chunk_points, N)
    cs = surv[:, :S].sum(axis=1).astype(np.int64)
    dropped = live & ~in_lead & (cs + (N - S) <= lead_max) & ((S - cs) * thr2 > lead_min * (1.0 + margin))
    if cstar == chunks:
        dropped[:] = False
    return ~dropped


@pytest.mark.parametrize("rate", [0.0, 0.01, 0.05, 0.5])
def test_the_count_rule_drops_only_what_the_exact_rule_prunes(rate):
    rs = np.random.RandomState(int(1000 * rate) + 7)
    dropped_total = pruned_total = 0
    for ratio, N, H in TP.CASES:
        models, (r2, inl, live) = TP.list_of(ratio, N, H)
        surv = inl | (rs.rand(*inl.shape) < rate)
        for route in (SINGLE, GROUP):
            cp = PC.chunk_points(N, route)
            m = PC.prune_model(r2, inl, live, PC.THR ** 2, cp)
            sel = preselect(surv, live, PC.THR ** 2, cp, m["lead_max"], m["lead_min"], m["cstar"], m["chunks"])
            wrong = np.flatnonzero(~sel & m["kept"])
            assert len(wrong) == 0, (ratio, N, H, route, wrong[:5])
            dropped_total += int((~sel).sum())
            pruned_total += int((~m["kept"]).sum())
    print(f"survivors = inliers + {rate:.0%} of the others: dropped {dropped_total} of the {pruned_total} the exact rule prunes")
    if rate == 0.0:
        # survivors = inliers: only the residual sum tells the two rules apart
        assert dropped_total > 0.9 * pruned_total


def flagship_survivors(seed, count):
    """(r2, inl, surv, live, chunk_points) of `count` oracle P3P models on the flagship scene of `seed`; survivors from the host
    build of the fp16 form in index order"""
    d = synth.absolute_pose_scene(5000, 0.7, seed)
    x = np.ascontiguousarray((np.asarray(d["p2d"]) - 500.0) / PC.FOCAL)
    X = np.ascontiguousarray(np.asarray(d["p3d"], float))
    N = len(x)
    sc = PC.Scene.__new__(PC.Scene)
    sc.a, sc.b = x, X
    models = sc.p3p_models(N, count, 300 + seed)
    cols = [x[:, 0], x[:, 1], X[:, 0], X[:, 1], X[:, 2]]
    xy = float(np.abs(x).max())
    thr2 = PC.THR ** 2
    live = ~np.isnan(models).any(axis=1)
    r2 = np.full((count, N), np.inf)
    inl = np.zeros((count, N), bool)
    surv = np.zeros((count, N), bool)
    for k in np.flatnonzero(live):
        rec = HM.pose_record(models[k][:4], models[k][4:])
        _, _, inl[k], r2[k] = HM.score("abs", rec, cols, thr2)
        en, out = HM.prefilter16_abs(rec, cols, thr2, xy, 0)
        assert en
        surv[k] = ~out
    assert not (inl & ~surv).any()
    return r2, inl, surv, live, PC.chunk_points(N, GROUP)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_flagship_pre_selection_keeps_at_most_twice_the_exact_rule(seed):
    r2, inl, surv, live, cp = flagship_survivors(seed, 2 * PC.LEAD)
    thr2 = PC.THR ** 2
    m = PC.prune_model(r2, inl, live, thr2, cp)
    assert m["cstar"] < m["chunks"]
    sel = preselect(surv, live, thr2, cp, m["lead_max"], m["lead_min"], m["cstar"], m["chunks"])
    assert not (~sel & m["kept"]).any()
    behind = live & (np.cumsum(live) > PC.LEAD)
    exact, pre = int((m["kept"] & behind).sum()), int((sel & behind).sum())
    print(f"seed {seed}: c* {m['cstar']} / {m['chunks']}, behind the lead {int(behind.sum())} live, exact rule keeps {exact}, "
          f"pre-selection keeps {pre} ({pre / max(exact, 1):.2f} x), survivors / inliers of the non-inlier pairs "
          f"{(surv & ~inl).sum() / (~inl[live]).sum():.4f}")
    assert pre <= 2 * exact
