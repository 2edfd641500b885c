"""The 1D-radial path of the device headers, compiled for the host (tests/hostmath_radial1d), against
tests/golden/golden_radial1d_v1.json - outputs of the reference's own sources recorded by tests/golden/make_golden_radial1d.py:
minimal solver, score, mask and refiner bit for bit.  Needs no GPU and no reference build."""
import json
import subprocess

import numpy as np
import pytest

import hostmath_radial1d_lib as HR
from golden import make_golden_radial1d as GR

G = json.load(open(GR.PATH))
LOSS_IDS = {"TRIVIAL": 0, "TRUNCATED": 1, "HUBER": 2, "CAUCHY": 3}


def floats(v):
    return np.array([float(x) for x in v])


def test_p5lp_radial_equals_the_reference_bit_for_bit():
    """240 samples - consistent, disturbed, un-normalised, planar (the NaN second root), repeated, identical and zero points: the number
    of models (the size of the reference's output, not its return value) and every pose"""
    xs, Xs, tags = GR.solver_samples()
    want = G["solver"]
    assert GR.digest([xs, Xs]) == want["input_sha256"], "the inputs changed: regenerate the fixture"
    counts, poses, nan = HR.p5lp_radial(xs, Xs)
    assert counts.tolist() == want["counts"]
    assert {0, 2, 4} <= set(want["counts"]) and "planar" in tags and "repeated" in tags
    for s, rec in enumerate(want["poses"]):
        if rec == "non-finite":
            assert not np.isfinite(poses[s, :counts[s]]).all() and nan[s, :counts[s]].any(), s
        else:
            assert GR.sample_digest(poses[s], counts[s]) == rec, (s, tags[s])
            assert not nan[s, :counts[s]].any()
            assert (poses[s, :counts[s], 6] == 0).all()  # t_z
    for s, rec in want["first"].items():
        assert GR.reprs(poses[int(s), :counts[int(s)]]) == rec, s
    assert all(c <= r for c, r in zip(want["counts"], want["returns"]))  # a root whose quadratic has no real solution gives no model


def test_sample_points_are_divided_by_their_norm():
    """absolute_pose.cc:357 `.normalized()`: x / sqrt(x . x), not x * (1 / sqrt(x . x))"""
    rs = np.random.RandomState(3)
    x = rs.randn(2000, 2) * 10.0 ** rs.uniform(-3, 3, (2000, 1))
    n = np.sqrt(0.0 + x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1])
    got = HR.normalized2(x)
    assert (got == x / n[:, None]).all()
    assert (got != x * (1.0 / n)[:, None]).any()


@pytest.mark.parametrize("n", GR.SCORE_N)
def test_score_count_and_mask_equal_the_reference_bit_for_bit(n):
    """ground truth, near, far, the ground truth turned by 180 degrees (alpha < 0) and a pose with a NaN"""
    want = G["scores"][str(n)]
    d, x, scale = GR.score_scene(n)
    assert GR.digest([x, d["p3d"]]) == want["pixels_sha256"], "the inputs changed: regenerate the fixture"
    assert repr(scale) == want["scale"]
    thr = float(want["max_error"])
    for name, pose in GR.score_poses(d, n).items():
        rec = want["poses"][name]
        s, cnt, mask = HR.score(pose, x, d["p3d"], thr)
        assert (repr(s), cnt, GR.mask_hex(mask)) == (rec["score"], rec["count"], rec["mask_hex"]), name
    assert want["poses"]["nan"]["count"] == 0 and want["poses"]["turned"]["count"] <= 0.1 * n


@pytest.mark.parametrize("n", GR.REFINE_N)
@pytest.mark.parametrize("run", sorted(GR.REFINE_RUNS))
def test_refiner_equals_the_reference_bit_for_bit(n, run):
    """Radial1DAbsolutePoseRefiner under TRUNCATED / 25 (the local optimisation) and CAUCHY / 100 (the final bundle's default): pose,
    costs and iteration count with every sum in correspondence order - what k_lm does up to 256 correspondences and k_lm_ordered at
    every size, 257 and 1000 included"""
    d, x, scale, p0 = GR.refine_inputs(n)
    want = G["refine"][f"{n}/{run}"]
    assert GR.digest([x, d["p3d"], p0]) == want["input_sha256"], "the inputs changed: regenerate the fixture"
    loss, iters = GR.REFINE_RUNS[run]
    pose, it, c0, c1 = HR.refine(p0, x, d["p3d"], HR.lm_options(iters, LOSS_IDS[loss], GR.MAX_ERROR * scale))
    assert it == want["iterations"]
    assert (repr(c0), repr(c1)) == (want["initial_cost"], want["cost"])
    assert GR.reprs(pose) == want["pose"]
    assert pose[6] == 0.0  # t_z is never touched


def test_solver_scorer_and_refiner_run_clean_under_the_sanitizers(tmp_path):
    """a stand-alone program (its own main, built with -fsanitize=address,undefined, started as a child process) over the fixture's
    solver samples, one score / pre-filter pass and one refinement"""
    exe = HR.check_program()
    xs, Xs, _ = GR.solver_samples()
    S = xs.shape[0]
    d, x, scale, p0 = GR.refine_inputs(257)
    blob = np.r_[float(S), np.concatenate([xs.reshape(S, 10), Xs.reshape(S, 15)], axis=1).ravel(), float(x.shape[0]), p0, x.ravel(),
                 d["p3d"].ravel(), GR.MAX_ERROR * scale]
    path = tmp_path / "in.bin"
    np.ascontiguousarray(blob, dtype=np.float64).tofile(path)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == ""
    assert r.stdout.startswith("models %d " % sum(G["solver"]["counts"]))
    assert " iterations %d " % G["refine"]["257/truncated"]["iterations"] in r.stdout


def test_generator_steps_equal_generate_models_bit_for_bit():
    """what k_generate<EST_RAD1D> does per lane - the sample's pixels divided by their norm, then the solver - on the fixture's scene
    (pixels that are not unit vectors) and samples: counts and poses of the reference's generate_models"""
    want = G["generate"]
    d, x, idx = GR.generate_inputs()
    assert GR.digest([x, d["p3d"], idx]) == want["input_sha256"], "the inputs changed: regenerate the fixture"
    xs = HR.normalized2(x[idx].reshape(-1, 2)).reshape(-1, 5, 2)
    counts, poses, nan = HR.p5lp_radial(xs, d["p3d"][idx])
    assert counts.tolist() == want["counts"] and not nan.any()
    for s, w in enumerate(want["poses"]):
        assert GR.sample_digest(poses[s], counts[s]) == w, s
    for s, w in want["first"].items():
        assert GR.reprs(poses[int(s), :counts[int(s)]]) == w, s


def test_filter_model_skips_by_the_entries_the_score_reads():
    """a NaN in t_z or in the quaternion-free third row is not read by the score: the host model of the kernel's entry test scores
    such a pose like the kernel does; a NaN in t_x skips it"""
    d, x, scale = GR.score_scene(64)
    gt = GR.gt_pose(d)
    thr = GR.MAX_ERROR * scale
    st0, rej0, inl0 = HR.prefilter(gt, x, d["p3d"], thr)
    tz = gt.copy()
    tz[6] = np.nan
    st, rej, inl = HR.prefilter(tz, x, d["p3d"], thr)
    assert (st, rej.tolist(), inl.tolist()) == (st0, rej0.tolist(), inl0.tolist()) and st == 1 and inl.sum() > 30
    tx = gt.copy()
    tx[4] = np.nan
    st, rej, inl = HR.prefilter(tx, x, d["p3d"], thr)
    assert st == 0 and rej.all() and not inl.any()
