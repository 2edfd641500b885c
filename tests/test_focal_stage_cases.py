"""The cases of tests/focal_stage_cases.py reach what they are there for - checked on the CPU, from the oracle alone, so that the
device tests (tests/test_gpu_focal_stages.py) compare bits of inputs that are known to sit on the kernels' edges."""
import numpy as np
import pytest

import focal_stage_cases as F
import oracle_lib as O


def test_kernel_constants_are_the_ones_the_sizes_were_chosen_for():
    assert (F.WAVE, F.ROUND, F.SOLVE_WAVES, F.SWITCH) == (64, 192, 4, 1024)
    assert F.MAX_MODELS == (10, 60) and F.SAMPLE == (4, 6)
    assert F.NS == (1, 63, 64, 65, 191, 192, 193, 384, 385, 500)
    assert F.GEN_BS == (1, 3, 4, 5, 63, 64, 65, 257)
    assert F.SLOT_COUNTS == (1, 5, 1024, 1025)
    assert [B * 10 for B in F.GATED_BS[0]] == [1020, 1030] and [B * 60 for B in F.GATED_BS[1]] == [1020, 1080]
    assert np.float64(F.FILL).tobytes() == b"\x5a" * 8


@pytest.mark.parametrize("which", F.WHICH)
def test_models_cover_the_kinds_of_hypothesis_a_run_meets(which):
    labels, M = F.models(which)
    n = F.N_SCENE
    counts, values = F.expected_scores(which, n)
    by = {g: [i for i, l in enumerate(labels) if l == g] for g in F.MODEL_GROUPS}
    assert len(by["hypothesis"]) == 20 and len(by["truth"]) == 4 and len(by["focal"]) == 3 and len(by["nan"]) == 3
    assert np.median(counts[by["hypothesis"]]) < 0.2 * n          # the oracle's own hypotheses: most have few inliers
    assert (counts[by["truth"]] > 0.4 * n).all() and counts[by["truth"]].max() >= 0.59 * n  # 40 % outliers: the rest fit the truth
    assert len(set(counts[by["truth"]].tolist())) > 1             # ... and the perturbations move some across the threshold
    assert [M[i, 7] for i in by["focal"]][0] == 0.0 and M[by["focal"][1], 7] < 0 and np.isposinf(M[by["focal"][2], 7])
    assert [int(np.flatnonzero(np.isnan(M[i]))[0]) for i in by["nan"]] == [1, 4, 7]
    assert (counts[by["nan"]] == 0).all()                          # (a NaN residual is no inlier)
    a, b = F.points(which, n)
    if which == 0:
        assert len(by["behind"]) == 1
        r2 = F.score_of(0, M[by["behind"][0]], a, b, F.THR2[0]).r2
        assert 0 < np.isnan(r2).sum() < n                          # part of the scene behind the camera, part in front
        assert np.isnan(values[by["nan"]]).sum() == 0              # (the inlier sum of no inliers is 0.0)
    else:
        assert np.allclose(values[by["nan"]], n * F.THR2[1], rtol=1e-12)  # (every correspondence pays the threshold, one after the other)
    # the sizes: the same model list has different counts at different n, so a scorer that stopped early or ran on would show
    for i in by["truth"]:
        assert len({int(F.expected_scores(which, m)[0][i]) for m in F.NS}) >= 6


@pytest.mark.parametrize("which", F.WHICH)
def test_inlier_patterns_lie_exactly_where_they_are_planted(which):
    seen = set()
    for p in F.patterns(which):
        sc = F.score_of(which, p.model, p.a, p.b, F.THR2[which])
        mask, _ = F.mask_of(which, p.model, p.a, p.b, F.THR2[which])
        assert np.array_equal(np.flatnonzero(sc.r2 < F.THR2[which]), p.inliers), (p.name, p.n)
        assert np.array_equal(np.flatnonzero(mask), p.inliers) and sc.count == len(p.inliers), (p.name, p.n)
        seen.add((p.name, tuple(p.inliers.tolist())) if len(p.inliers) <= 2 else (p.name, p.n))
    names = {p.name for p in F.patterns(which)}
    assert names == {"first", "last", "all", "none", "wave edge", "round edge", "beyond the first round"}
    assert ("wave edge", (63, 64)) in seen and ("round edge", (191, 192)) in seen and ("first", (0,)) in seen
    assert {p.n for p in F.patterns(which) if p.name == "beyond the first round"} == {193, 385, 500}
    assert {int(p.inliers[0]) for p in F.patterns(which) if p.name == "last"} == {n - 1 for n in F.PATTERN_NS}


@pytest.mark.parametrize("which", F.WHICH)
def test_a_threshold_on_a_residual_excludes_the_point_and_the_next_double_includes_it(which):
    cases = F.ties(which)
    assert len(cases) == 12 and {t.stage for t in cases} == {"score", "mask"}
    a, b = F.points(which, F.TIE_N)
    for out, inn in zip(cases[0::2], cases[1::2]):
        assert out.k == inn.k and not out.inside and inn.inside and inn.thr2 == np.nextafter(out.thr2, np.inf)
        if out.stage == "score":
            so, si = F.score_of(which, out.model, a, b, out.thr2), F.score_of(which, inn.model, a, b, inn.thr2)
            assert so.r2[out.k] == out.thr2 and si.count == so.count + 1
        else:
            (mo, r2), (mi, _) = F.mask_of(which, out.model, a, b, out.thr2), F.mask_of(which, inn.model, a, b, inn.thr2)
            assert r2[out.k] == out.thr2 and not mo[out.k] and mi[out.k] and mi.sum() == mo.sum() + 1
    assert {t.k for t in cases} == set(F.TIE_POINTS) or all(abs(t.k - w) <= 8 for t, w in zip(cases[0::2], F.TIE_POINTS * 2))


def test_reciprocal_and_division_disagree_often_enough_to_be_tested():
    cases, counted_only, masked_only = F.splits()
    assert counted_only >= F.SPLITS_EACH_WAY and masked_only >= F.SPLITS_EACH_WAY, (counted_only, masked_only)
    assert sum(c.counted for c in cases) == F.SPLITS_EACH_WAY and sum(c.masked for c in cases) == F.SPLITS_EACH_WAY
    a, b = F.points(0, F.SPLIT_N)
    for c in cases:
        sc = F.score_of(0, c.model, a, b, c.thr2)
        mask, r2m = F.mask_of(0, c.model, a, b, c.thr2)
        assert (sc.r2[c.k] < c.thr2) == c.counted and bool(mask[c.k]) == c.masked and c.counted != c.masked
        assert abs(sc.r2[c.k] - r2m[c.k]) <= 1e-12 * c.thr2  # (rounding of one reciprocal, amplified by f z / z2 - x)


def test_the_focal_length_filter_meets_every_sub_case():
    bounds = F.max_focals()
    assert bounds["none"] == -1.0 and bounds["zero"] == 0.0 and bounds["median"] > 0
    sol = F.solver_output(F.FILTER_N)
    # P3.5Pf's focal length is (|row 1| + |row 2|) / 2 of the projection matrix times the mean norm of the image points (p35pf.cc:
    # 60-62, :913-917): it is never negative, so the filter's first line (focal < 0) has no sample to drop - here or in any scene.
    # The rule stays in apply_filter and is held against the estimator below; a NaN focal length passes both lines on both sides.
    assert not any(bool((f < 0).any()) for _, f in sol)
    for name, bound in bounds.items():
        g = F.generated(0, F.FILTER_N, bound)
        for i, (poses, focals) in enumerate(sol):                  # the three-line rule on the solver's output = the estimator
            want = F.apply_filter(poses, focals, bound)
            assert g.counts[i] == len(want) and np.array_equal(g.models[i, : len(want)], want, equal_nan=True), (name, i)
    g = F.generated(0, F.FILTER_N, bounds["median"])
    full = np.array([len(f) for _, f in sol])
    assert ((g.counts == 0) & (full > 0)).any()                    # some samples lose all of their solutions
    assert ((g.counts == full) & (full > 1)).any()                 # some keep all of them
    moved = 0
    for i, (poses, focals) in enumerate(sol):
        keep = [not focals[j] < 0 and not focals[j] > bounds["median"] for j in range(len(focals))]
        moved += any(not keep[j] and any(keep[j + 1:]) for j in range(len(keep)))
    assert moved > 0                                               # some lose a solution that is not the last: later ones move forward
    total = F.generated(0, F.FILTER_N).counts.sum()
    assert 0.3 * total < g.counts.sum() < 0.7 * total              # about half are dropped
    assert F.generated(0, F.FILTER_N, 0.0).counts.sum() == 0
    # the bound that equals a solution's focal length keeps it
    e = F.generated(0, F.FILTER_N, bounds["equal"])
    assert (e.models[..., 7] == bounds["equal"]).any() and e.counts.sum() < total
    assert not (e.models[..., 7] > bounds["equal"]).any()


@pytest.mark.parametrize("which", F.WHICH)
def test_generator_problems_make_the_sampler_redraw_and_yield_models(which):
    K = F.SAMPLE[which]
    for n in F.GEN_NS[which]:
        g = F.generated(which, n)
        steps = np.diff(g.positions.astype(np.int64))
        assert (steps >= K).all() and (g.samples < n).all()
        assert all(len(set(s.tolist())) == K for s in g.samples)
        if n <= K + 1:
            assert (steps > K).mean() > 0.5                        # duplicates redrawn in most samples
        assert g.counts.sum() > 0 and g.counts.max() <= F.MAX_MODELS[which]
    g = F.generated(which, 300)
    assert len(set(g.counts[: 65].tolist())) > 2                   # iterations with different numbers of models


@pytest.mark.parametrize("which", F.WHICH)
def test_gated_batches_have_empty_full_and_partial_iterations_on_both_sides_of_the_switch(which):
    for B in F.GATED_BS[which]:
        slots, num, idx = F.gated(which, B)
        maxm = F.MAX_MODELS[which]
        assert slots.shape == (B * maxm, 8) and (num == 0).any() and (num == maxm).any() and ((num > 0) & (num < maxm)).any()
        assert ((idx >= 0).reshape(B, maxm).sum(axis=1) == num).all()
        assert set(idx[idx >= 0].tolist()) == set(range(len(F.models(which)[1])))  # every model of the list sits in a filled slot
    assert F.GATED_BS[which][0] * F.MAX_MODELS[which] <= F.SWITCH < F.GATED_BS[which][1] * F.MAX_MODELS[which]
    assert min(F.SLOT_COUNTS) == 1 and F.SWITCH in F.SLOT_COUNTS and F.SWITCH + 1 in F.SLOT_COUNTS
    models, idx = F.padded(which, F.SWITCH + 1)
    assert np.array_equal(models[: F.SWITCH], F.padded(which, F.SWITCH)[0], equal_nan=True) and idx.max() == len(F.models(which)[1]) - 1


def test_oracle_exports_agree_with_each_other():
    """the inlier sum plus the outliers' charge is the MSAC value; the mask's count is the score's where the two forms agree"""
    a, b = F.points(0, 385)
    for m in F.models(0)[1][:24]:
        isum, cnt, r2, msac = O.score_image(m[:7], m[7], a, b, F.THR2[0])
        assert msac == isum + float(len(a) - cnt) * F.THR2[0]
        assert cnt == int(np.sum(r2 < F.THR2[0]))
