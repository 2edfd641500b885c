"""The rule of the pruned matrix-core absolute-pose scorer on the CPU: a numpy model of the lead, the selection and the finalize
(tests/prune_cases.py) on the oracle's inlier flags and per-point residuals.

Over random and planted lists: the candidate set of the records_body rule on the values a pruned step reports equals the set on the
full values, and no pruned hypothesis has a true count above, or a true score below, the running values at its position.  Then the
gate and the arithmetic of the split chunk at its clamps.  The inputs of tests/test_gpu_score_prune.py are checked here as well: the
set the device has to prune at least is large enough that the device test cannot pass by never pruning."""
import numpy as np
import pytest

import prune_cases as PC
from poselib_amd import api

THR2 = PC.THR ** 2


def _check_list(r2, inl, live, chunk_points, init_max=0, init_min=PC.DBL_MAX):
    m = PC.prune_model(r2, inl, live, THR2, chunk_points, init_max, init_min)
    full = PC.records_rule(m["full_counts"], m["full_scores"], init_max, init_min)
    got = PC.records_rule(m["counts"], m["scores"], init_max, init_min)
    assert got == full, (sorted(set(got) ^ set(full))[:5], m["cstar"])
    # running values in front of every position, on the full values
    emax = np.maximum.accumulate(np.r_[init_max, m["full_counts"]])[:-1]
    emin = np.minimum.accumulate(np.r_[init_min, m["full_scores"]])[:-1]
    pr = ~m["kept"]
    assert (m["full_counts"][pr] <= emax[pr]).all()
    assert (m["full_scores"][pr] >= emin[pr]).all()
    # what a pruned hypothesis reports is a count not above and a score not below its full values
    assert (m["counts"][pr] <= m["full_counts"][pr]).all() and (m["scores"][pr] >= m["full_scores"][pr] * (1 - 1e-12)).all()
    assert (m["counts"][~pr] == m["full_counts"][~pr]).all()
    return m


@pytest.mark.parametrize("ratio", [0.1, 0.7, 1.0])
def test_candidates_of_random_lists_are_unchanged(ratio):
    sc = PC.scene(ratio)
    N = 1281
    models = sc.p3p_models(N, PC.LEAD + 1500, 31)
    r2, inl, live = PC.reference(sc, N, models)
    pruned = 0
    for chunk_points in (64, 256, 320):  # many chunks, and the two shapes of the launches
        for lead in (0, 1):  # the whole list as it is, and behind an incumbent as good as its best
            best = (int(inl.sum(axis=1).max()), float((np.where(inl, r2, 0).sum(axis=1) + (N - inl.sum(axis=1)) * THR2).min()))
            m = _check_list(r2, inl, live, chunk_points, *((0, PC.DBL_MAX) if lead == 0 else best))
            pruned += int((~m["kept"]).sum())
            if ratio == 1.0 and lead == 0:
                assert m["cstar"] == m["chunks"] and m["kept"].all()
    if ratio < 1.0:
        assert pruned > 0


def test_planted_lists():
    sc = PC.scene(0.7)
    N = 1281
    models = sc.p3p_models(N, PC.LEAD + 600, 32)
    r2, inl, live = PC.reference(sc, N, models)
    cnt = inl.sum(axis=1)
    wrong = np.flatnonzero(live & (cnt < 30))
    good = PC.perturbed_gt(sc, 1e-6, 5)
    # a lead without a good model, the only good one behind it: nothing can be pruned before it is seen, it is kept and listed
    lst = np.vstack([models[wrong[:PC.LEAD + 40]], good[None], models[wrong[PC.LEAD + 40:PC.LEAD + 80]]])
    m = _check_list(*PC.reference(sc, N, lst), 320)
    k = PC.LEAD + 40
    assert m["kept"][k] and k in PC.records_rule(m["counts"], m["scores"])
    # a model behind the lead whose count equals the lead's best exactly (a copy of it): kept, and listed as today
    best = int(np.argmax(np.where(live & (np.cumsum(live) <= PC.LEAD), cnt, -1)))
    lst = np.vstack([models, models[best][None]])
    m = _check_list(*PC.reference(sc, N, lst), 320)
    assert m["full_counts"][-1] == m["lead_max"] and m["kept"][-1]
    # an incumbent better than anything in the list: everything behind the lead may go, nothing is listed
    m = _check_list(r2, inl, live, 320, init_max=N, init_min=1e-12)
    assert PC.records_rule(m["counts"], m["scores"], N, 1e-12) == []
    assert (~m["kept"]).sum() == (live & (np.cumsum(live) > PC.LEAD)).sum()
    # NaN models only: no live hypothesis, c* = chunks
    lst = np.array([PC.nan_model(models[k], k) for k in range(70)])
    m = _check_list(*PC.reference(sc, N, lst), 320)
    assert m["cstar"] == m["chunks"] and m["kept"].all()


def test_split_chunk_at_the_clamps():
    f = PC.split_chunk
    N, cp = 1281, 320
    assert f(0, PC.DBL_MAX, N, THR2, cp, 5) == 5          # no incumbent, empty lead
    assert f(0, N * THR2, N, THR2, cp, 5) == 5            # a lead without inliers: need = N + margin
    assert f(N, 0.0, N, THR2, cp, 5) == 1                 # everything an inlier without error: need = margin, one chunk at least
    assert f(0xffffffff, 0.0, N, THR2, cp, 5) == 1        # (the group diagnostic's incumbent count)
    assert f(N - 320 + PC.MARGIN_POINTS, 0.0, N, THR2, cp, 5) == 1   # need = 320: the first chunk holds it exactly
    assert f(N - 321 + PC.MARGIN_POINTS, 0.0, N, THR2, cp, 5) == 2   # one more correspondence: two chunks
    assert f(N - 1280 + PC.MARGIN_POINTS, 0.0, N, THR2, cp, 5) == 4  # need = 1280: four full chunks ...
    assert f(N - 1280 + PC.MARGIN_POINTS - 1, 0.0, N, THR2, cp, 5) == 5  # ... 1281 = N: not below N, every chunk
    assert f(1000, 100.5 * THR2, N, THR2, cp, 5) == 1     # the score's bound decides: 100.5 + 32 < 320 ...
    assert f(1000, 300.0 * THR2, N, THR2, cp, 5) == 2     # ... 332 > 320


def test_gate():
    for n, it, want in [(5000, 8192, True), (5000, 8191, False), (5000, 100000, True), (1100, 10000, True), (1024, 8192, True),
                        (1023, 100000, False), (200, 100000, False), (700, 16384, False), (5000, 4096, False), (5000, 1000, False)]:
        assert api.score_prune_gate(0, n, it) == want == PC.prune_gate(0, n, it), (n, it)
    for kind in (1, 2, 3):
        assert not api.score_prune_gate(kind, 5000, 100000)
    # every size the matrix-core scorer takes has at least three chunks, so the iteration count decides there
    assert api.score_shape(0, 1024, True, False)[0] >= 3 and api.score_shape(0, 1023, True, False) is None


def test_device_cases_cannot_pass_by_never_pruning():
    """the lists of tests/test_gpu_score_prune.py: what the model prunes with a doubled margin - the set the device has to prune at
    least - is more than half of the long lists, and most of what lies behind the lead of the short ones at 70 % outliers"""
    import test_gpu_score_prune as T

    for ratio, N, H in T.LONG:
        for route in (PC.SINGLE, PC.GROUP):
            m = T.model_of(ratio, N, H, route, margin=2e-6)
            assert (~m["kept"]).sum() > H // 2, (ratio, N, H, route, int((~m["kept"]).sum()))
            assert 1 <= m["cstar"] < m["chunks"]
    m = T.model_of(0.7, PC.N_MAX, T.LENGTHS[-1], PC.SINGLE, margin=2e-6)
    assert 1 < m["cstar"] < m["chunks"] - 1  # the split in the middle
    assert T.model_of(1.0, 1281, T.LENGTHS[-1], PC.SINGLE)["cstar"] == 5
