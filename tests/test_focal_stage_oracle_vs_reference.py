"""Pins the oracle's stage exports of the two focal-length estimators (oracle_lib.score_image, inliers_image, score_shared_focal,
inliers_shared_focal, generate_focal) to the REFERENCE'S OWN SOURCES (oracle/_ref, tests/ref_lib.py) bit for bit, on the cases the device
tests use (tests/focal_stage_cases.py): compute_msac_score(Image) and get_inliers(Image), the Sampson score and mask of F = K_inv (E
K_inv), the two estimators' generate_models on the same samples.  The reference returns no per-point residual; the oracle's are
pinned through the thresholds placed on them: at thr2 = r2 of point k the reference leaves k out, at the next double it takes it.
Skipped where neither the reference's sources nor a prebuilt library are present."""
import numpy as np
import pytest

import focal_stage_cases as F
import oracle_lib as O
import ref_lib as R

pytestmark = pytest.mark.skipif(not R.available(), reason="reference build (oracle/_ref) not available")


def bits_equal(got, want):
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    return got.shape == want.shape and bool(((got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))).all())


def reference_score(which, m, a, b, thr2):
    """(MSAC score, count) of the reference"""
    with np.errstate(all="ignore"), R.reference():
        if which == 0:
            _, cnt, _, msac = O.score_image(m[:7], m[7], a, b, thr2)
        else:
            msac, cnt, _ = O.score_shared_focal(m[:7], m[7], a, b, thr2)
    return msac, cnt


def oracle_score(which, m, a, b, thr2):
    with np.errstate(all="ignore"):
        if which == 0:
            _, cnt, _, msac = O.score_image(m[:7], m[7], a, b, thr2)
        else:
            msac, cnt, _ = O.score_shared_focal(m[:7], m[7], a, b, thr2)
    return msac, cnt


def reference_mask(which, m, a, b, thr2):
    with R.reference():
        return F.mask_of(which, m, a, b, thr2)[0]


@pytest.mark.parametrize("which", F.WHICH)
def test_scores_and_masks_of_every_model_at_every_size(which):
    for n in F.NS:
        a, b = F.points(which, n)
        for i, m in enumerate(F.models(which)[1]):
            (so, co), (sr, cr) = oracle_score(which, m, a, b, F.THR2[which]), reference_score(which, m, a, b, F.THR2[which])
            assert co == cr and bits_equal(so, sr), (n, i, so, sr)
            assert np.array_equal(F.mask_of(which, m, a, b, F.THR2[which])[0], reference_mask(which, m, a, b, F.THR2[which])), (n, i)


@pytest.mark.parametrize("which", F.WHICH)
def test_inlier_patterns(which):
    for p in F.patterns(which):
        (so, co), (sr, cr) = oracle_score(which, p.model, p.a, p.b, F.THR2[which]), reference_score(which, p.model, p.a, p.b, F.THR2[which])
        assert co == cr == len(p.inliers) and bits_equal(so, sr), (p.name, p.n)
        assert np.array_equal(np.flatnonzero(reference_mask(which, p.model, p.a, p.b, F.THR2[which])), p.inliers), (p.name, p.n)


@pytest.mark.parametrize("which", F.WHICH)
def test_thresholds_on_a_residual_pin_the_per_point_values(which):
    a, b = F.points(which, F.TIE_N)
    for t in F.ties(which):
        if t.stage == "score":
            (so, co), (sr, cr) = oracle_score(which, t.model, a, b, t.thr2), reference_score(which, t.model, a, b, t.thr2)
            assert co == cr and bits_equal(so, sr), t
        mo, mr = F.mask_of(which, t.model, a, b, t.thr2)[0], reference_mask(which, t.model, a, b, t.thr2)
        assert np.array_equal(mo, mr) and (t.stage != "mask" or bool(mr[t.k]) == t.inside), t
    for out, inn in zip(F.ties(which)[0::2], F.ties(which)[1::2]):
        if out.stage == "score":  # the reference's own count moves by exactly the point
            assert reference_score(which, inn.model, a, b, inn.thr2)[1] == reference_score(which, out.model, a, b, out.thr2)[1] + 1


def test_reciprocal_against_division():
    a, b = F.points(0, F.SPLIT_N)
    for c in F.splits()[0]:
        (so, co), (sr, cr) = oracle_score(0, c.model, a, b, c.thr2), reference_score(0, c.model, a, b, c.thr2)
        assert co == cr and bits_equal(so, sr), c
        mr = reference_mask(0, c.model, a, b, c.thr2)
        assert np.array_equal(F.mask_of(0, c.model, a, b, c.thr2)[0], mr) and bool(mr[c.k]) == c.masked, c
        # the reference itself counts the point and masks it out, or the other way round: remove it and the count moves or does not
        keep = np.arange(F.SPLIT_N) != c.k
        assert cr - reference_score(0, c.model, a[keep], b[keep], c.thr2)[1] == int(c.counted), c


@pytest.mark.parametrize("which", F.WHICH)
def test_generate_on_the_sampler_s_samples(which):
    bounds = F.max_focals().values() if which == 0 else [-1.0]
    # (the reference's six-point coefficients call std::pow(d, 3): the oracle in the same mode - its default is the device's cube)
    with O.libm_cubes():
        for n in F.GEN_NS[which]:
            g = F.generated(which, n)
            for bound in (bounds if n == F.FILTER_N else [-1.0]):
                with np.errstate(all="ignore"):
                    co, mo = O.generate_focal(which, g.a, g.b, g.samples, bound)
                    with R.reference():
                        cr, mr = O.generate_focal(which, g.a, g.b, g.samples, bound)
                assert np.array_equal(co, cr) and bits_equal(mo, mr), (n, bound)
