"""GPU parity (-m gpu) of 1D-radial absolute pose (estimate_1D_radial_absolute_pose) through the C-ABI / poselib_amd, against
tests/golden/golden_radial1d_v1.json - outputs of the reference's own sources, recorded on the CPU by
tests/golden/make_golden_radial1d.py (the reference build is not available next to a GPU).

Everything is held bit for bit: solver, scores, masks, refinements (beyond 256 correspondences with the sums in the reference's
order, pl_set_lm_mode(1); in the default mode the iteration counts and the pose within 1e-6, the project's standard for tree sums),
and every recorded estimator case."""
import json

import numpy as np
import pytest

import lm_cases as LC
from golden import make_golden_radial1d as GR
from poselib_amd import synth

pytestmark = pytest.mark.gpu

G = json.load(open(GR.PATH))


def floats(v):
    return np.array([float(x) for x in v])


def pose7(p):
    return np.r_[p.q, p.t]


# ------------------------------------------------------------------------------------------ minimal solver
def test_p5lp_radial_through_solve_batch_equals_the_reference(gpu):
    """k_solve_batch<EST_RAD1D> - the solver the generator kernel runs per lane - on the fixture's 240 samples, the planar, repeated,
    identical and zero ones included: number of models and every pose; pl_p5lp_radial gives the same for single samples"""
    xs, Xs, tags = GR.solver_samples()
    want = G["solver"]
    assert GR.digest([xs, Xs]) == want["input_sha256"], "the inputs changed: regenerate the fixture"
    first = np.concatenate([xs, np.zeros(xs.shape[:2] + (1,))], axis=2)
    rec, cnt = gpu.solve_batch(gpu.KIND_RAD1D, first, Xs)
    assert cnt.tolist() == want["counts"]
    for s, w in enumerate(want["poses"]):
        poses = rec[s, :, :7]
        if w == "non-finite":
            assert not np.isfinite(poses[:cnt[s]]).all(), s
        else:
            assert GR.sample_digest(poses, cnt[s]) == w, (s, tags[s])
    for s in (0, 2, 3, 4):
        single = gpu.p5lp_radial(xs[s], Xs[s])
        assert len(single) == cnt[s]
        assert GR.reprs(np.array([pose7(p) for p in single])) == GR.reprs(rec[s, :cnt[s], :7]), s


# ------------------------------------------------------------------------------------------ score, mask
@pytest.mark.parametrize("n", GR.SCORE_N)
def test_score_and_mask_of_the_recorded_poses_bit_for_bit(gpu, n):
    """k_score_seq<EST_RAD1D> and k_mask<EST_RAD1D>: ground truth, near, far, turned by 180 degrees (alpha < 0), a NaN entry"""
    want = G["scores"][str(n)]
    d, x, scale = GR.score_scene(n)
    assert GR.digest([x, d["p3d"]]) == want["pixels_sha256"], "the inputs changed: regenerate the fixture"
    thr = float(want["max_error"])
    P = gpu.Problem(gpu.KIND_RAD1D, x, d["p3d"])
    for name, pose in GR.score_poses(d, n).items():
        rec = want["poses"][name]
        cp = gpu.CameraPose(pose[:4], pose[4:])
        score, count = P.score(cp, thr)
        mask = gpu.inlier_mask(P, cp, thr)
        print(n, name, "count", count, "score", repr(score), "recorded", rec["count"], rec["score"])
        assert (repr(score), count, GR.mask_hex(mask)) == (rec["score"], rec["count"], rec["mask_hex"]), name
    P.close()


# ------------------------------------------------------------------------------------------ streaming scorer
STREAM_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
import poselib_amd as P
import test_gpu_radial1d as T
out = {}
for n in T.stream_sizes(P):
    for H in T.STREAM_MODELS:
        cnt, sc, path = T.stream_run(P, n, H)
        out["%d/%d" % (n, H)] = [[int(c) for c in cnt], [repr(float(s)) for s in sc], int(path)]
print("RESULT " + json.dumps(out))
"""
STREAM_MODELS = [1, 63, 64, 65, 200]


def stream_sizes(P):
    """5, one below, at and one above the scorer's chunk size as built, and 1000"""
    from poselib_amd import _lib

    chunk = int(_lib.lib().pl_debug_radial1d_chunk())
    assert 8 <= chunk <= 512
    return [5, chunk - 1, chunk, chunk + 1, 1000]


def stream_inputs(n):
    d, x, scale = GR.scaled_scene(n, 0.0 if n <= 5 else 0.3, 9700 + n)
    return d, x, GR.MAX_ERROR * scale


def stream_models(d, H):
    """the ground truth disturbed at every scale from 1e-6 to 1 (good models keep hundreds of pairs, bad ones a handful), a pose with a
    NaN in t_x, one with a NaN in t_z (which the score does not read) and the ground truth turned by 180 degrees among them"""
    rs = np.random.RandomState(1000 + H)
    gt = GR.gt_pose(d)
    M = np.zeros((H, 7))
    for k in range(H):
        s = 10.0 ** rs.uniform(-6, 0)
        q = gt[:4] + s * rs.randn(4)
        M[k] = np.r_[q / np.linalg.norm(q), gt[4:6] + s * rs.randn(2), 0.0]
    M[0] = gt
    if H > 3:
        M[H // 2, 4] = np.nan
        M[H - 2] = GR.score_poses(d, 0)["turned"]
        M[H - 1] = gt
        M[H - 1, 6] = np.nan
    return M


def stream_run(P, n, H):
    d, x, thr = stream_inputs(n)
    pr = P.Problem(P.KIND_RAD1D, x, d["p3d"])
    cnt, sc, path = pr.score_stream(stream_models(d, H), thr)
    pr.close()
    return cnt.copy(), sc.copy(), path


def test_streaming_scorer_equals_the_sequential_scorer_with_and_without_the_filter(gpu):
    """k_score_radial1d (fp32 pre-filter, queue, exact drain) against k_score_seq<EST_RAD1D>: the same counts for 1, 63, 64, 65 and 200
    models on 5, chunk - 1, chunk, chunk + 1 and 1000 correspondences; the scores agree to the rounding of a sum of n terms in another
    order (n 2^-52 of the score: every term is non-negative).  The same runs in a fresh process with POSELIB_AMD_NO_PREFILTER=1 (every
    pair evaluated exactly) give the same bits: the filter only removes work."""
    import os
    import subprocess
    import sys

    got = {}
    filtered = 0
    for n in stream_sizes(gpu):
        d, x, thr = stream_inputs(n)
        pr = gpu.Problem(gpu.KIND_RAD1D, x, d["p3d"])
        for H in STREAM_MODELS:
            M = stream_models(d, H)
            cnt, sc, path = pr.score_stream(M, thr)
            filtered += path == 1
            for k in range(H):
                s, c = pr.score(gpu.CameraPose(M[k, :4], M[k, 4:]), thr)
                assert cnt[k] == c, (n, H, k, cnt[k], c)
                assert abs(sc[k] - s) <= (n + 64) * 2.0 ** -52 * s, (n, H, k, sc[k], s)
            if H > 3:
                assert cnt[H // 2] == 0 and cnt[H - 2] <= 0.1 * n  # NaN in t_x; turned
                assert cnt[H - 1] == cnt[0]  # NaN in t_z: not read
            if n >= 64:
                assert cnt[0] >= 0.5 * n
            got["%d/%d" % (n, H)] = [[int(c) for c in cnt], [repr(float(s)) for s in sc], int(path)]
        pr.close()
    assert filtered == len(got) or os.environ.get("POSELIB_AMD_NO_PREFILTER")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", STREAM_CHILD, root], env=dict(os.environ, POSELIB_AMD_NO_PREFILTER="1"), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    exact = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert all(v[2] == 0 for v in exact.values())  # the child did run without the filter
    assert {k: v[:2] for k, v in exact.items()} == {k: v[:2] for k, v in got.items()}


# ------------------------------------------------------------------------------------------ refinement
@pytest.mark.parametrize("n", GR.REFINE_N)
@pytest.mark.parametrize("run", sorted(GR.REFINE_RUNS))
def test_refinement_equals_the_reference(gpu, n, run):
    """Refiner<EST_RAD1D> (pl_refine_model with kind 5 = bundle_adjust_1D_radial): with the sums in the reference's order - k_lm up to
    256 correspondences, k_lm_ordered (pl_set_lm_mode(1)) beyond - pose bit for bit; in the default mode beyond 256 (tree sums)
    identical iteration counts, the pose within 1e-6 and the bits recorded in tests/golden/lm_tree_bits_v1.json"""
    want = G["refine"][f"{n}/{run}"]
    d, x, scale, p0 = GR.refine_inputs(n)
    assert GR.digest([x, d["p3d"], p0]) == want["input_sha256"], "the inputs changed: regenerate the fixture"
    got, it, pr, p0, bundle = GR.refine_on_device(gpu, n, run)
    ref = floats(want["pose"])
    print(n, run, "default mode: iterations", it, want["iterations"], "max |pose difference|", float(np.abs(got - ref).max()))
    assert it == want["iterations"]
    if n <= 256:
        assert GR.reprs(got) == want["pose"]
    else:
        assert np.abs(got - ref).max() < 1e-6
        LC.assert_pinned("rad1d", f"{n}/{run}", got, it)
        before = gpu.set_lm_mode(1)
        try:
            pose, it = pr.refine(gpu.CameraPose(p0[:4], p0[4:]), bundle)
        finally:
            gpu.set_lm_mode(before)
        assert it == want["iterations"]
        assert GR.reprs(pose7(pose)) == want["pose"]
        got = pose7(pose)
    assert got[6] == 0.0
    pr.close()


# ------------------------------------------------------------------------------------------ estimator
def api_options(opt):
    o = {k: (dict(v) if isinstance(v, dict) else v) for k, v in opt.items()}
    o.get("ransac", {}).pop("score_initial_model", None)  # (set by passing an initial pose)
    return o


def estimate_case(gpu, name):
    case = [c for c in GR.EST_CASES if c[0] == name][0]
    rec = G["estimates"][name]
    d, opt, initial = GR.est_inputs(case, rec["data_seed"])
    assert GR.digest([d["p2d"], d["p3d"]]) == rec["input_sha256"], "the inputs changed: regenerate the fixture"
    init = None if initial is None else gpu.CameraPose(initial[:4], initial[4:])
    pose, info = gpu.estimate_1D_radial_absolute_pose(d["p2d"], d["p3d"], api_options(opt), init)
    return rec, d, opt, initial, pose, info


@pytest.mark.parametrize("name", [c[0] for c in GR.EST_CASES if c[1] >= 5])
def test_estimate_takes_the_references_decisions(gpu, name):
    """every recorded case - 30 %, 60 % and 50 % outliers at 400, 400 and 2000 correspondences, n = 5, 6, 7, 12, PROSAC, a warm start:
    iterations, refinements, num_inliers, model_score and mask of the reference's run and its pose bit for bit, with the refinements'
    sums in the reference's order (pl_set_lm_mode(1): above 256 correspondences the default mode's tree sums move a refined pose by
    1e-13)"""
    before = gpu.set_lm_mode(1)
    try:
        rec, d, opt, initial, pose, info = estimate_case(gpu, name)
    finally:
        gpu.set_lm_mode(before)
    n = rec["n"]
    mask = np.unpackbits(np.frombuffer(bytes.fromhex(rec["mask_hex"]), dtype=np.uint8))[:n].astype(bool)
    ref = floats(rec["model"])
    print(name, "iterations", info["iterations"], rec["iterations"], "refinements", info["refinements"], rec["refinements"], "inliers",
          info["num_inliers"], rec["num_inliers"], "max |pose difference|", float(np.abs(pose7(pose) - ref).max()))
    assert (info["iterations"], info["refinements"], info["num_inliers"]) == (rec["iterations"], rec["refinements"], rec["num_inliers"])
    assert (np.array(info["inliers"]) == mask).all()
    assert repr(info["model_score"]) == rec["model_score"]
    assert GR.reprs(pose7(pose)) == rec["model"]
    assert pose.t[2] == 0.0


def test_estimate_in_the_default_mode(gpu):
    """n = 400 at 30 % outliers with the default summation order (tree sums above 256 correspondences): the reference's decisions and
    mask, its pose within 1e-6"""
    rec, d, opt, initial, pose, info = estimate_case(gpu, "n400_o30")
    mask = np.unpackbits(np.frombuffer(bytes.fromhex(rec["mask_hex"]), dtype=np.uint8))[:rec["n"]].astype(bool)
    assert (info["iterations"], info["refinements"], info["num_inliers"]) == (rec["iterations"], rec["refinements"], rec["num_inliers"])
    assert (np.array(info["inliers"]) == mask).all()
    assert np.abs(pose7(pose) - floats(rec["model"])).max() < 1e-6
    assert GR.recovers(d, pose7(pose), mask)


def test_too_few_points_give_default_stats_and_an_untouched_pose(gpu):
    """n = 4 (robust.cc:892-895): nothing runs"""
    rec = G["estimates"]["n4"]
    assert (rec["iterations"], rec["refinements"], rec["num_inliers"]) == (0, 0, 0)
    case = [c for c in GR.EST_CASES if c[0] == "n4"][0]
    d, opt, _ = GR.est_inputs(case, rec["data_seed"])
    start = gpu.CameraPose([0.5, 0.5, -0.5, 0.5], [0.25, -2.0, 3.0])
    pose, info = gpu.estimate_1D_radial_absolute_pose(d["p2d"], d["p3d"], api_options(opt), start)
    assert (info["iterations"], info["refinements"], info["num_inliers"]) == (0, 0, 0)
    assert pose7(pose).tolist() == [0.5, 0.5, -0.5, 0.5, 0.25, -2.0, 3.0]
    assert not any(info["inliers"])


def test_ransac_stage_through_its_three_routes(gpu):
    """pl_ransac_1D_radial_pnp and the resident problem (pl_problem_create kind 5 + pl_ransac_run) on the rescaled pixels equal each
    other bit for bit and the front-end's RANSAC stage in iterations, refinements, inliers, score and mask"""
    rec, d, opt, initial, pose, info = estimate_case(gpu, "n400_o60")
    scale = GR.front_scale(d["p2d"])
    xs = d["p2d"] * scale
    o = api_options(opt)
    o["max_error"] = GR.MAX_ERROR * scale
    p1, i1 = gpu.ransac_1D_radial_pnp(xs, d["p3d"], o)
    pr = gpu.Problem(gpu.KIND_RAD1D, xs, d["p3d"])
    p2, i2 = pr.run(o)
    pr.close()
    assert GR.reprs(pose7(p1)) == GR.reprs(pose7(p2))
    for key in ("iterations", "refinements", "num_inliers", "inliers"):
        assert i1[key] == i2[key] == info[key], key
    assert repr(i1["model_score"]) == repr(i2["model_score"]) == repr(info["model_score"])
    assert p1.t[2] == 0.0


def test_batch_item_runs_solo_and_equals_its_single_call(gpu):
    """one 1D-radial item among absolute-pose items of pl_estimate_batch: every result equals the single call bit for bit, and the
    report counts the 1D-radial item under `solo`"""
    problems, singles = [], []
    for k in range(4):
        a = synth.absolute_pose_scene(400 + 5 * k, 0.3, 9950 + k)
        oa = {"max_error": 2.0, "ransac": {"seed": k}}
        problems.append(("abs", a["p2d"], a["p3d"], a["camera"], oa))
        img, info = gpu.estimate_absolute_pose(a["p2d"], a["p3d"], a["camera"], oa)
        singles.append((img.pose, info))
        if k == 1:
            r = synth.radial_1d_scene(350, 0.3, 9960)
            orad = {"max_error": 2.0, "ransac": {"seed": 3}}
            problems.append(("radial1d", r["p2d"], r["p3d"], orad))
            singles.append(gpu.estimate_1D_radial_absolute_pose(r["p2d"], r["p3d"], orad))
    out = gpu.estimate_batch(problems)
    report = gpu.last_batch_report()
    print(report)
    assert report["items"] == 5 and report["solo"] == 1
    for k, ((m, info), (m1, info1)) in enumerate(zip(out, singles)):
        pose = m.pose if hasattr(m, "pose") else m
        assert GR.reprs(pose7(pose)) == GR.reprs(pose7(m1)), k
        for key in ("iterations", "refinements", "num_inliers", "inliers"):
            assert info[key] == info1[key], (k, key)
        assert repr(info["model_score"]) == repr(info1["model_score"]), k


# ------------------------------------------------------------------------------------------ generator kernel
def generate_problem(gpu):
    d, x, idx = GR.generate_inputs()
    assert GR.digest([x, d["p3d"], idx]) == G["generate"]["input_sha256"], "the inputs changed: regenerate the fixture"
    return d, x, idx, gpu.Problem(gpu.KIND_RAD1D, x, d["p3d"])


def test_generator_kernel_on_explicit_samples_equals_generate_models(gpu):
    """k_generate<EST_RAD1D> itself (pl_debug_radial1d_generate: a resident problem, explicit samples as PROSAC hands them over): the
    gather from the point set, the normalisation of the sample's pixels on the device (the scene's pixels are not unit vectors), the
    solver, the records and the per-block accounting - counts and every pose of the reference's generate_models on the same samples"""
    want = G["generate"]
    d, x, idx, pr = generate_problem(gpu)
    rec, cnt, (total, nan_models, overflow) = gpu.radial1d_generate(pr, idx, 4)
    pr.close()
    assert cnt.tolist() == want["counts"]
    for s, w in enumerate(want["poses"]):
        assert GR.sample_digest(rec[s, :, :7], cnt[s]) == w, s
    for s, w in want["first"].items():
        assert GR.reprs(rec[int(s), :cnt[int(s)], :7]) == w, s
    assert (total, nan_models, overflow) == (sum(want["counts"]), 0, 0)
    # the record's matrix is R(q) of the stored quaternion, slots beyond the count stay untouched
    for s in range(len(cnt)):
        assert (rec[s, cnt[s]:] == 0).all()


def test_generator_kernel_reports_an_overflow_of_its_slots(gpu):
    """slots_per_iter = 2: an iteration with 4 solutions sets gen_overflow and counts 0 (the host repeats such a batch with more room);
    the iterations that fit are unchanged"""
    want = G["generate"]
    d, x, idx, pr = generate_problem(gpu)
    rec, cnt, (total, nan_models, overflow) = gpu.radial1d_generate(pr, idx, 2)
    pr.close()
    assert 4 in want["counts"] and overflow == 1
    expect = [0 if c > 2 else c for c in want["counts"]]
    assert cnt.tolist() == expect and total == sum(expect)
    for s, w in enumerate(want["poses"]):
        if want["counts"][s] <= 2:
            assert GR.sample_digest(rec[s, :, :7], cnt[s]) == w, s


def test_generator_kernel_with_a_nan_point(gpu):
    """a correspondence with a NaN pixel: every sample that holds it gives no model (NaN coefficients have no real root), as in the
    reference; the others are unchanged.  No input was found that makes the solver emit a pose with a NaN entry, so the NaN-model
    count of the accounting stays 0 here: that branch of the kernel is NOT exercised on the device by any test."""
    want = G["generate"]
    d, x, idx = GR.generate_inputs()
    bad = int(idx[0, 0])
    xn = x.copy()
    xn[bad, 0] = np.nan
    pr = gpu.Problem(gpu.KIND_RAD1D, xn, d["p3d"])
    rec, cnt, (total, nan_models, overflow) = gpu.radial1d_generate(pr, idx, 4)
    pr.close()
    holds = (idx == bad).any(axis=1)
    assert holds[0] and (cnt[holds] == 0).all()
    assert cnt[~holds].tolist() == [c for c, h in zip(want["counts"], holds) if not h]
    assert (nan_models, overflow) == (0, 0) and total == int(cnt.sum())


# ------------------------------------------------------------------------------------------ pl_ransac_batch, sharded run
def test_ransac_batch_item_runs_solo_and_equals_problem_run(gpu):
    """a kind-5 problem among absolute-pose problems of pl_ransac_batch: the result of its own pl_ransac_run, reported solo"""
    r = synth.radial_1d_scene(350, 0.3, 9961)
    scale = GR.front_scale(r["p2d"])
    probs = [gpu.Problem(gpu.KIND_RAD1D, r["p2d"] * scale, r["p3d"])]
    opts = [{"max_error": GR.MAX_ERROR * scale, "ransac": {"seed": 5}}]
    for k in range(3):
        a = synth.absolute_pose_scene(400 + 5 * k, 0.3, 9970 + k)
        f, cx, cy = a["camera"]["params"]
        probs.append(gpu.Problem(gpu.KIND_ABS, (a["p2d"] - [cx, cy]) / f, a["p3d"]))
        opts.append({"max_error": 2.0 / f, "ransac": {"seed": k}})
    singles = [p.run(o) for p, o in zip(probs, opts)]
    out = gpu.ransac_batch(probs, opts)
    report = gpu.last_batch_report()
    print(report)
    assert report["items"] == 4 and report["solo"] == 1
    for k, ((m, info), (m1, info1)) in enumerate(zip(out, singles)):
        assert GR.reprs(pose7(m)) == GR.reprs(pose7(m1)), k
        for key in ("iterations", "refinements", "num_inliers", "inliers"):
            assert info[key] == info1[key], (k, key)
        assert repr(info["model_score"]) == repr(info1["model_score"]), k
    for p in probs:
        p.close()


def test_sharded_run_is_unsupported(gpu):
    r = synth.radial_1d_scene(50, 0.0, 9962)
    pr = gpu.Problem(gpu.KIND_RAD1D, r["p2d"], r["p3d"])
    with pytest.raises(gpu.PoseLibAmdError, match="error -4"):
        pr.run_sharded({"max_error": 2.0}, 0, 1, lambda s, rcv: None)
    pr.close()
