"""The matrix-core absolute-pose scorer runs over the LIVE hypotheses only (-m gpu).

k_score_mfma streams the hypotheses whose record carries no NaN flag (a stable compaction of the hypothesis list, built by
k_compact2 / k_live_list), writes its partial sums per live position, and k_finalize2 maps them back through rank[]: a NaN
model gets count 0 and score N thr^2 without having been scored.  The fp16 operand rows of the correspondences come from a
table that is rebuilt with the threshold of every launch sequence.  Checked here, at N = 1100 correspondences (above the
1024 below which the matrix-core path is off; 4 chunks of 320, the last one with 140 valid columns):

* NaN models anywhere in a list (none, scattered, whole units of 64 at either end, all, all but one) x list lengths around the
  32- and 64-hypothesis unit boundaries: counts equal the oracle's exact evaluation, NaN models score exactly N thr^2, an
  infinite translation is NOT a NaN model, and the finite models score as they do without the NaN ones around them;
* one problem scored and run at several thresholds in turn: operands of an earlier threshold would drop or admit the
  correspondences planted at the decision boundaries;
* whole runs (13 % NaN hypotheses) against the oracle, and the grouped batch path against the single runs bit for bit.
"""
import numpy as np
import pytest

import oracle_lib as O
from poselib_amd import synth
from test_gpu_full_size import FOCAL, _abs_models, _model_diff, _plant_at_threshold

pytestmark = pytest.mark.gpu

N = 1100
THR = 0.012
LENGTHS = [1, 31, 32, 33, 64, 65, 129, 200]
PATTERNS = ["none", "every_8th", "first_70", "last_70", "all", "all_but_64", "good_after_64"]
INF_AT = 3  # index of the model with an infinite translation in the base list


@pytest.fixture(scope="module")
def scene():
    """the correspondences, 200 finite models (ground truth, perturbed, random, one infinite translation) and their oracle
    scores - computed once, shared by every case"""
    rs = np.random.RandomState(4100)
    d = synth.absolute_pose_scene(N, 0.5, 4101)
    x = (np.asarray(d["p2d"]) - 500.0) / FOCAL
    X = np.asarray(d["p3d"], float)
    base = []
    while len(base) < max(LENGTHS):
        base.extend(_abs_models(d, 1.0, np.zeros(3), rs))
    base = np.array(base[: max(LENGTHS)])
    base[INF_AT, 4:] = [0.0, np.inf, 1.0]
    ref = [O.score("reproj", m, x, X, THR * THR) for m in base]
    return x, X, base, ref


def _nan_model(m, which):
    m = m.copy()
    if which % 3 == 0:
        m[1] = np.nan  # in q
    elif which % 3 == 1:
        m[4 + (which // 3) % 3] = np.nan  # in one component of t only
    else:
        m[0] = m[6] = np.nan  # in both
    return m


def _nan_mask(pattern, n):
    m = np.zeros(n, bool)
    if pattern == "every_8th":
        m[::8] = True
    elif pattern == "first_70":
        m[:70] = True
    elif pattern == "last_70":
        m[-70:] = True
    elif pattern == "all":
        m[:] = True
    elif pattern == "all_but_64":
        m[:] = True
        m[min(64, n - 1)] = False
    elif pattern == "good_after_64":
        m[: min(64, n - 1)] = True
    return m


@pytest.mark.parametrize("pattern", PATTERNS)
def test_nan_models_anywhere_in_the_list(gpu, scene, pattern):
    x, X, base, ref = scene
    prob = gpu.Problem(gpu.KIND_ABS, x, X)
    for n in LENGTHS:
        nan = _nan_mask(pattern, n)
        M = base[:n].copy()
        want = list(ref[:n])
        if pattern in ("all_but_64", "good_after_64"):  # the survivor / the model behind the run: the ground truth
            g = min(64, n - 1)
            M[g], want[g] = base[0], ref[0]
        for k in np.flatnonzero(nan):
            M[k] = _nan_model(M[k], k)
        cnt, sc, path = prob.score_stream(M, THR)
        assert path == 2, (pattern, n, path)
        for k in range(n):
            if nan[k]:
                assert cnt[k] == 0 and sc[k] == float(N) * THR * THR, (pattern, n, k, cnt[k], sc[k])
                osc, ocnt = O.score("reproj", M[k], x, X, THR * THR)
                assert ocnt == 0 and osc == sc[k]
            else:
                osc, ocnt = want[k]
                assert cnt[k] == ocnt, (pattern, n, k, cnt[k], ocnt)
                assert abs(sc[k] - osc) <= 1e-9 * abs(osc) + 1e-300, (pattern, n, k, sc[k], osc)
        if n > INF_AT and not nan[INF_AT] and not (pattern in ("all_but_64", "good_after_64") and min(64, n - 1) == INF_AT):
            assert np.isinf(M[INF_AT]).any() and cnt[INF_AT] == ref[INF_AT][1]  # infinite, not NaN: evaluated
        if (~nan).any() and nan.any():  # the same finite models without the NaN ones around them
            cnt2, sc2, path2 = prob.score_stream(M[~nan], THR)
            assert path2 == 2
            assert (np.asarray(cnt2) == np.asarray(cnt)[~nan]).all(), (pattern, n)
    prob.close()
    if pattern == "good_after_64":
        assert ref[0][1] > N // 4  # the model behind the run of NaN does have inliers


def test_one_problem_scored_and_run_at_several_thresholds(gpu):
    rs = np.random.RandomState(4200)
    d = synth.absolute_pose_scene(N, 0.5, 4201)
    x = (np.asarray(d["p2d"]) - 500.0) / FOCAL
    X = np.asarray(d["p3d"], float)
    M = np.array(_abs_models(d, 1.0, np.zeros(3), rs))
    # half of the correspondences at the first model's decision boundary - a sixth for each of the three thresholds
    thrs = [0.012, 0.5, 0.012, 1e-3, 0.012]
    pick = rs.randint(0, 6, N)
    for j, thr in enumerate((0.012, 0.5, 1e-3)):
        planted = _plant_at_threshold(M[0, :4], M[0, 4:], X, thr, rs)
        x[pick == j] = planted[pick == j]
    prob = gpu.Problem(gpu.KIND_ABS, x, X)
    ref = {thr: [O.score("reproj", m, x, X, thr * thr) for m in M] for thr in set(thrs)}
    for thr in thrs:
        cnt, sc, path = prob.score_stream(M, thr)
        assert path == 2, (thr, path)
        for k in range(len(M)):
            osc, ocnt = ref[thr][k]
            assert cnt[k] == ocnt, (thr, k, cnt[k], ocnt)
            assert abs(sc[k] - osc) <= 1e-9 * abs(osc) + 1e-300
    # ... and two runs with different thresholds on the same problem
    for err in (0.012, 0.004, 0.012):
        opt = {"max_error": err, "ransac": {"max_iterations": 2000, "min_iterations": 2000, "seed": 7}}
        model, info = prob.run(opt)
        want, mask, st = O.ransac_pnp(x, X, opt)
        assert info["hypotheses"] == st["hypotheses"] and info["refinements"] == st["refinements"]
        assert info["num_inliers"] == st["num_inliers"]
        assert (np.array(info["inliers"]) == mask).all()
        assert _model_diff(0, model, want) <= 1e-6
    prob.close()


def _run_scene(seed):
    d = synth.absolute_pose_scene(N, 0.7, seed)
    return (np.asarray(d["p2d"]) - 500.0) / FOCAL, np.asarray(d["p3d"], float)


def _run_opt(seed):
    return {"max_error": 0.012, "ransac": {"max_iterations": 2000, "min_iterations": 2000, "seed": seed}}


@pytest.fixture(scope="module")
def single_runs(gpu):
    out = {}
    for seed in (31, 32):
        x, X = _run_scene(seed)
        prob = gpu.Problem(gpu.KIND_ABS, x, X)
        out[seed] = (x, X, prob.run(_run_opt(seed)))
        prob.close()
    return out


@pytest.mark.parametrize("seed", [31, 32])
def test_run_with_nan_hypotheses_matches_the_oracle(gpu, single_runs, seed):
    x, X, (model, info) = single_runs[seed]
    want, mask, st = O.ransac_pnp(x, X, _run_opt(seed))
    print("seed", seed, "hypotheses", info["hypotheses"], "nan", info["nan_hypotheses"], "inliers", info["num_inliers"],
          "refinements", info["refinements"])
    assert info["iterations"] == st["iterations"] == 2000
    assert info["refinements"] == st["refinements"]
    assert info["hypotheses"] == st["hypotheses"]
    assert info["num_inliers"] == st["num_inliers"]
    assert (np.array(info["inliers"]) == mask).all()
    assert _model_diff(0, model, want) <= 1e-6
    assert info["nan_hypotheses"] > 0


def test_live_list_over_several_scan_blocks_matches_the_oracle(gpu):
    """k_compact2 starts the live positions of every block of 1024 iterations at the generators' NaN counts of the blocks in
    front of it: 4500 iterations are five blocks, the last one partial"""
    x, X = _run_scene(31)
    opt = _run_opt(31)
    opt["ransac"].update(max_iterations=4500, min_iterations=4500)
    prob = gpu.Problem(gpu.KIND_ABS, x, X)
    model, info = prob.run(opt)
    prob.close()
    want, mask, st = O.ransac_pnp(x, X, opt)
    assert info["iterations"] == st["iterations"] == 4500
    assert info["hypotheses"] == st["hypotheses"] and info["refinements"] == st["refinements"]
    assert info["num_inliers"] == st["num_inliers"]
    assert (np.array(info["inliers"]) == mask).all()
    assert _model_diff(0, model, want) <= 1e-6
    assert info["nan_hypotheses"] > 0


def test_grouped_runs_equal_the_single_runs_bit_for_bit(gpu, single_runs):
    seeds = [31, 32, 31, 32, 31]  # group size 4: one full and one partial group
    probs = [gpu.Problem(gpu.KIND_ABS, single_runs[s][0], single_runs[s][1]) for s in seeds]
    got = gpu.ransac_batch(probs, [_run_opt(s) for s in seeds], 2, 4)
    for s, p, (m, info) in zip(seeds, probs, got):
        wm, winfo = single_runs[s][2]
        for key in ("iterations", "refinements", "hypotheses", "nan_hypotheses", "num_inliers", "model_score"):
            assert info[key] == winfo[key], (s, key, info[key], winfo[key])
        assert (np.array(info["inliers"]) == np.array(winfo["inliers"])).all()
        assert (np.r_[m.q, m.t] == np.r_[wm.q, wm.t]).all()
        p.close()
