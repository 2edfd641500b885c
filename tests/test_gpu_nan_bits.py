"""NaN flags of an iteration as one dense word written by the P3P generator (-m gpu).

k_compact2 builds the live hypothesis list from GenerateArgs::nan_bits - bit m of entry i: model m of iteration i carries the NaN
flag - instead of reading the flag word of every record.  The runs below have about 13 % NaN models (N = 1100, 70 % outliers)
and lengths at the wavefront (64) and scan-block (1024) edges of the generator and of the scan.  Everything behind the live
list (hypotheses, inliers, mask, model) must be the oracle's; the oracle keeps no count of NaN models, so nan_hypotheses is
compared between the paths.  The grouped path - the generator's grouped entry, and its entry for PROSAC's host-drawn samples -
must equal the single runs bit for bit."""
import numpy as np
import pytest

import oracle_lib as O
from test_gpu_full_size import FOCAL, _model_diff
from poselib_amd import synth

pytestmark = pytest.mark.gpu

N = 1100
ITERATIONS = [1, 63, 64, 65, 1023, 1024, 1025, 2049]
KEYS = ("iterations", "refinements", "hypotheses", "nan_hypotheses", "num_inliers", "model_score", "inlier_ratio")
POSE_TOL = 1e-6


def _opt(iterations, seed, **ransac):
    return {"max_error": 0.012, "ransac": dict({"max_iterations": iterations, "min_iterations": iterations, "seed": seed}, **ransac)}


@pytest.fixture(scope="module")
def points():
    d = synth.absolute_pose_scene(N, 0.7, 6100)
    x = (np.asarray(d["p2d"]) - 500.0) / FOCAL
    X = np.asarray(d["p3d"], float)
    order = np.argsort(~d["inlier_gt"], kind="stable")  # inliers first: a quality order for PROSAC
    return x, X, order


@pytest.fixture(scope="module")
def single_runs(gpu, points):
    x, X, _ = points
    prob = gpu.Problem(gpu.KIND_ABS, x, X)
    out = {it: prob.run(_opt(it, 40 + k)) for k, it in enumerate(ITERATIONS)}
    prob.close()
    return out


@pytest.mark.parametrize("iterations", ITERATIONS)
def test_single_run_matches_the_oracle(points, single_runs, iterations):
    x, X, _ = points
    model, info = single_runs[iterations]
    want, mask, st = O.ransac_pnp(x, X, _opt(iterations, 40 + ITERATIONS.index(iterations)))
    print("iterations", iterations, "hypotheses", info["hypotheses"], "nan", info["nan_hypotheses"], "inliers", info["num_inliers"])
    assert info["iterations"] == st["iterations"] == iterations
    assert info["hypotheses"] == st["hypotheses"]
    assert info["num_inliers"] == st["num_inliers"]
    assert (np.array(info["inliers"]) == mask).all()
    assert _model_diff(0, model, want) <= POSE_TOL


def test_the_runs_do_have_nan_models(single_runs):
    assert single_runs[2049][1]["nan_hypotheses"] > 100  # ~13 % of ~2700
    assert sum(single_runs[it][1]["nan_hypotheses"] for it in (63, 64, 65)) > 0


def _same(tag, got, want):
    (m, info), (wm, winfo) = got, want
    for key in KEYS:
        assert info[key] == winfo[key], (tag, key, info[key], winfo[key])
    assert info["inliers"] == winfo["inliers"], tag
    assert (np.r_[m.q, m.t] == np.r_[wm.q, wm.t]).all(), tag


def test_one_batch_call_equals_the_single_runs_bit_for_bit(gpu, points, single_runs):
    x, X, _ = points
    probs = [gpu.Problem(gpu.KIND_ABS, x, X) for _ in ITERATIONS]
    got = gpu.ransac_batch(probs, [_opt(it, 40 + k) for k, it in enumerate(ITERATIONS)], 2, len(ITERATIONS))
    for it, g in zip(ITERATIONS, got):
        _same(it, g, single_runs[it])
    for p in probs:
        p.close()


def test_prosac_member_of_a_group_equals_its_single_run(gpu, points, single_runs):
    """PROSAC's samples are drawn on the host and uploaded: the generator reads them instead of drawing"""
    x, X, order = points
    xs, Xs = x[order], X[order]
    popt = _opt(1025, 77, progressive_sampling=True)
    prob = gpu.Problem(gpu.KIND_ABS, xs, Xs)
    want = prob.run(popt)
    prob.close()
    ref, mask, st = O.ransac_pnp(xs, Xs, popt)
    assert want[1]["hypotheses"] == st["hypotheses"] and want[1]["iterations"] == st["iterations"]
    assert want[1]["num_inliers"] == st["num_inliers"] and (np.array(want[1]["inliers"]) == mask).all()
    probs = [gpu.Problem(gpu.KIND_ABS, xs, Xs), gpu.Problem(gpu.KIND_ABS, x, X), gpu.Problem(gpu.KIND_ABS, x, X)]
    got = gpu.ransac_batch(probs, [popt, _opt(1025, 46), _opt(64, 42)], 1, 3)
    _same("prosac", got[0], want)
    _same(1025, got[1], single_runs[1025])
    _same(64, got[2], single_runs[64])
    for p in probs:
        p.close()
