"""The fp32 pre-filter of the 1D-radial streaming scorer (pl_prefilter.h pf_radial1d_outlier) never rejects a pair the exact
expression accepts (r^2 < thr^2 and alpha > 0): over the fixture's scenes with good, disturbed and random models at every scale, and
over correspondences and thresholds of every magnitude.  Prints the share of non-inlier pairs that reach the exact pass.  Host
compile of the device headers (tests/hostmath_radial1d): needs no GPU."""
import numpy as np
import pytest

import hostmath_radial1d_lib as HR
from golden import make_golden_radial1d as GR


def models_at_every_scale(d, rs, count):
    gt = GR.gt_pose(d)
    out = [gt]
    for _ in range(count):
        s = 10.0 ** rs.uniform(-7, 0.5)
        q = gt[:4] + s * rs.randn(4)
        out.append(np.r_[q / np.linalg.norm(q), gt[4:6] + s * rs.randn(2), 0.0])
    for _ in range(count // 4):
        q = rs.randn(4)
        out.append(np.r_[q / np.linalg.norm(q), rs.randn(2) * 10.0 ** rs.uniform(-3, 3), 0.0])
    return out


@pytest.mark.parametrize("n", GR.SCORE_N + [400])
def test_filter_never_rejects_an_inlier_on_the_scenes(n):
    d, x, scale = GR.score_scene(n) if n in GR.SCORE_N else GR.scaled_scene(n, 0.5, 7290)
    rs = np.random.RandomState(7500 + n)
    thr = GR.MAX_ERROR * scale
    reach = total = inliers = 0
    for pose in models_at_every_scale(d, rs, 200):
        st, rej, inl = HR.prefilter(pose, x, d["p3d"], thr)
        assert st == 1
        assert not (rej & inl).any(), pose
        reach += int((~rej & ~inl).sum())
        total += int((~inl).sum())
        inliers += int(inl.sum())
    print("n", n, "inlier pairs", inliers, "non-inlier pairs", total, "of them reaching the exact pass: %.3f %%" % (100.0 * reach / max(total, 1)))
    assert inliers > 0


@pytest.mark.parametrize("exp", [-6, -3, 0, 3, 6])
def test_filter_never_rejects_an_inlier_at_any_magnitude(exp):
    """pixels, 3-D points, translations and thresholds scaled by powers of ten; thresholds from 1e-6 to 10 times the pixel scale"""
    rs = np.random.RandomState(7600 + exp)
    seen = 0
    for trial in range(40):
        d, x, scale = GR.scaled_scene(300, 0.4, 7700 + trial % 5)
        sx, sX = 10.0 ** (exp * rs.uniform(0, 1)), 10.0 ** (exp * rs.uniform(0, 1))
        xs, Xs = x * sx, d["p3d"] * sX
        gt = GR.gt_pose(d)
        for k in range(6):
            s = 0.0 if k == 0 else 10.0 ** rs.uniform(-6, 0)
            q = gt[:4] + s * rs.randn(4)
            pose = np.r_[q / np.linalg.norm(q), (gt[4:6] + s * rs.randn(2)) * sX, 0.0]
            thr = sx * 10.0 ** rs.uniform(-6, 1) / np.sqrt((x ** 2).sum(1)).mean()
            st, rej, inl = HR.prefilter(pose, xs, Xs, thr)
            assert st in (1, 2)
            assert not (rej & inl).any(), (trial, k, sx, sX, thr)
            seen += int(inl.sum())
    assert seen > 0


def test_nan_and_out_of_range_models():
    d, x, scale = GR.score_scene(64)
    gt = GR.gt_pose(d)
    nan = gt.copy()
    nan[5] = np.nan
    st, rej, inl = HR.prefilter(nan, x, d["p3d"], GR.MAX_ERROR * scale)
    assert st == 0 and not inl.any()
    st, rej, inl = HR.prefilter(gt * np.r_[1e30, 1e30, 1e30, 1e30, 1, 1, 1], x, d["p3d"], GR.MAX_ERROR * scale)
    assert st == 2 and not rej.any()
