"""Grouped scorer launches with the slice count taken from the work of the launch (-m gpu).

driver_group.inc picks the hypothesis slices of k_score_mfma_g per step from the chunks of all active members
(group_score_slices): a member of a large group of long runs gets fewer, longer-lived workgroups than the same member alone.
Which wavefront produces a (chunk, hypothesis) partial has no influence on it, so every pl_ransac_batch result must equal
pl_ransac_run's bit for bit whatever the group looks like: model, mask and every statistic.  N = 1100 is the smallest size on the
matrix-core path (4 chunks of 320 correspondences, the last one with 140 valid columns)."""
import numpy as np
import pytest

from poselib_amd import api, synth
from test_gpu_full_size import FOCAL

pytestmark = pytest.mark.gpu

KEYS = ("iterations", "refinements", "hypotheses", "nan_hypotheses", "num_inliers", "model_score", "inlier_ratio")
LONG = 100000
GROUP_SIZES = (1, 3, 16, 48)


def _scene(n, seed):
    d = synth.absolute_pose_scene(n, 0.7, seed)
    return (np.asarray(d["p2d"]) - 500.0) / FOCAL, np.asarray(d["p3d"], float)


def _fixed(iterations, seed):
    return {"max_error": 0.012, "ransac": {"max_iterations": iterations, "min_iterations": iterations, "seed": seed}}


def _assert_same(tag, got, want):
    (m, info), (wm, winfo) = got, want
    for key in KEYS:
        assert info[key] == winfo[key], (tag, key, info[key], winfo[key])
    assert info["inliers"] == winfo["inliers"], tag
    assert (np.r_[m.q, m.t] == np.r_[wm.q, wm.t]).all(), tag  # bit for bit


def _check_batch(gpu, members, group_size, in_flight=2):
    """members: (x, X, opt, single-run result)"""
    probs = [gpu.Problem(gpu.KIND_ABS, x, X) for x, X, _, _ in members]
    got = gpu.ransac_batch(probs, [opt for _, _, opt, _ in members], in_flight, group_size)
    for i, (g, (_, _, _, want)) in enumerate(zip(got, members)):
        _assert_same((group_size, i), g, want)
    for p in probs:
        p.close()


def _single(gpu, x, X, opt):
    p = gpu.Problem(gpu.KIND_ABS, x, X)
    out = p.run(opt)
    p.close()
    return out


@pytest.fixture(scope="module")
def long_members(gpu):
    """48 long runs at N = 1100 (four scenes, 48 seeds) and their single-problem results, computed once"""
    scenes = [_scene(1100, 5200 + k) for k in range(4)]
    out = []
    for i in range(48):
        x, X = scenes[i % 4]
        opt = _fixed(LONG, 900 + i)
        out.append((x, X, opt, _single(gpu, x, X, opt)))
    return out


def test_the_cases_cover_a_reduced_and_an_unreduced_launch():
    solo = api.group_slices(api.KIND_ABS, 1100, LONG, 4)
    per_size = {gs: api.group_slices(api.KIND_ABS, 1100, LONG, 4 * gs) for gs in GROUP_SIZES}
    print("slices per member, N = 1100,", LONG, "iterations:", per_size, "alone:", solo)
    assert any(s == solo for s in per_size.values()), per_size
    assert any(s < solo for s in per_size.values()), per_size


@pytest.mark.parametrize("group_size", GROUP_SIZES)
def test_long_runs_in_groups_of_every_size_equal_the_single_runs(gpu, long_members, group_size):
    _check_batch(gpu, long_members, group_size)


MIXED = [(n, LONG if i % 2 == 0 else 20000) for i, n in enumerate([1100, 2500, 5000] * 4)]  # (correspondences, iterations)


def _chunks(n):
    return -(-n // 320)


def test_the_mixed_group_holds_reduced_and_unreduced_members():
    lc = sum(_chunks(n) for n, _ in MIXED)
    got = [api.group_slices(api.KIND_ABS, n, it, lc) for n, it in MIXED]
    solo = [api.group_slices(api.KIND_ABS, n, it, _chunks(n)) for n, it in MIXED]
    print("mixed group, launch_chunks", lc, "slices", got, "alone", solo)
    assert any(g < s for g, s in zip(got, solo)), (got, solo)  # the long runs are cut coarser than alone ...
    assert any(g == s for g, s in zip(got, solo)), (got, solo)  # ... the short lists keep their count
    assert len(set(got)) > 1  # members of one launch below its max_slices


def test_one_group_of_mixed_sizes_equals_the_single_runs(gpu):
    members = []
    for i, (n, it) in enumerate(MIXED):
        x, X = _scene(n, 5300 + i)
        opt = _fixed(it, 700 + i)
        members.append((x, X, opt, _single(gpu, x, X, opt)))
    _check_batch(gpu, members, len(MIXED), in_flight=1)


# One group of N = 5000 members (16 chunks each) whose active set shrinks:
#   8 x min = max = 40000: the whole run is the group's first step (a batch holds up to min_iterations + 2 iterations);
#   4 x default options on an easy scene: stop after the first step;
#   3 x default min_iterations, max_iterations = 40000 on a 90 % outlier scene: 1001 iterations in the first step, then batches as
#       long as the stop rule's bound asks for - in launches that hold these three members only.
SHRINK_FIRST, SHRINK_LATER = 16 * 15, 16 * 3  # launch_chunks of the first step and of the later ones


def test_the_shrinking_group_goes_from_a_reduced_to_a_coarser_cut():
    alone = api.group_slices(api.KIND_ABS, 5000, 40000, 16)
    first = api.group_slices(api.KIND_ABS, 5000, 40000, SHRINK_FIRST)
    later = api.group_slices(api.KIND_ABS, 5000, 40000, SHRINK_LATER)
    print("N = 5000, 40000 iterations: alone", alone, "in the full launch", first, "with three members left", later)
    assert first < alone  # the first step's launch is reduced
    assert later > first  # the same batch gets more slices once twelve members have stopped


def test_members_that_stop_early_shrink_the_launch(gpu):
    """fixed 40000 iterations, default options and slow starters in one group (see above): the active set - and with it
    launch_chunks and the slice count the rule gives a batch - changes between steps"""
    members = []
    for i in range(15):
        kind = "fixed" if i < 8 else "default" if i < 12 else "slow"
        d = synth.absolute_pose_scene(5000, {"fixed": 0.7, "default": 0.4, "slow": 0.9}[kind], 5400 + i)
        x, X = (np.asarray(d["p2d"]) - 500.0) / FOCAL, np.asarray(d["p3d"], float)
        opt = _fixed(40000, 800 + i) if kind == "fixed" else {"max_error": 0.012, "ransac": {"seed": 800 + i}}
        if kind == "slow":
            opt["ransac"]["max_iterations"] = 40000
        want = _single(gpu, x, X, opt)
        print(kind, "iterations", want[1]["iterations"])
        if kind == "default":
            assert want[1]["iterations"] < 40000
        if kind == "slow":
            assert want[1]["iterations"] > 1100  # more than the first step's batch
        members.append((x, X, opt, want))
    _check_batch(gpu, members, 15, in_flight=1)
