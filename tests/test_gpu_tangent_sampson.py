"""GPU parity (-m gpu) of tangent-Sampson relative pose (RelativePoseOptions::tangent_sampson) through the C-ABI / poselib_amd,
against tests/golden/golden_tangent_v1.json - outputs of the reference's own sources, recorded on the CPU by
tests/golden/make_golden_tangent.py (the reference build is not available next to a GPU).

Standards, the project's existing ones (tests/test_gpu_radial_cameras.py): scores, masks and refinements of up to 256
correspondences bit for bit; identical LM iteration counts beyond and the pose within 1e-6.
"""
import json

import numpy as np
import pytest

import lm_cases as LC
from golden import make_golden_tangent as GT
from golden.make_golden import digest
from poselib_amd import synth

pytestmark = pytest.mark.gpu

G = json.load(open(GT.PATH))


def floats(v):
    return np.array([float(x) for x in v])


def tangent_problem(gpu, case):
    """the resident problem of one of the fixture's score scenes, from the scaled pixels and rescaled cameras"""
    name, m1, m2, n, outl, fov, seed = case
    d, x1, x2, c1, c2 = GT.scene(m1, m2, n, outl, fov, seed)
    assert digest([x1, x2]) == G["scores"][name]["pixels_sha256"], "the inputs changed: regenerate the fixture"
    scale, x1s, x2s, c1s, c2s = GT.scaled_inputs(x1, x2, c1, c2)
    return gpu.TangentProblem(x1s, x2s, c1s, c2s)


# ------------------------------------------------------------------------------------------ preparation, score, mask
@pytest.mark.parametrize("case", GT.SCORE_SCENES, ids=[c[0] for c in GT.SCORE_SCENES])
def test_prepared_problem_scores_the_recorded_poses_bit_for_bit(gpu, case):
    """d and M are computed on the device (k_prepare); count, score and mask of the ground truth, two perturbations of it, t = 0 and a
    pose with a NaN equal the reference's: k_score_seq<EST_RELT> and k_mask<EST_RELT> on the device's own bearings and Jacobians"""
    want = G["scores"][case[0]]
    P = tangent_problem(gpu, case)
    thr = float(want["max_error"])
    for name, rec in want["poses"].items():
        pose = floats(rec["pose"])
        score, count = P.score(gpu.CameraPose(pose[:4], pose[4:]), thr)
        mask = gpu.inlier_mask(P, gpu.CameraPose(pose[:4], pose[4:]), thr)
        print(case[0], name, "count", count, "score", repr(score), "recorded", rec["count"], rec["score"])
        assert (repr(score), count, GT.mask_hex(mask)) == (rec["score"], rec["count"], rec["mask_hex"]), name
    P.close()


# ------------------------------------------------------------------------------------------ rejections
def test_camera_model_outside_the_nine_is_unsupported(gpu):
    x = np.random.RandomState(1).rand(8, 2)
    with pytest.raises(gpu.PoseLibAmdError, match="error -4"):
        gpu.TangentProblem(x, x, {"model": 6, "params": [1.0, 1.0, 0.0, 0.0, 0.5]}, None)


def test_ransac_relpose_with_the_flag_is_unsupported(gpu):
    x = np.random.RandomState(2).rand(16, 2)
    with pytest.raises(gpu.PoseLibAmdError, match="error -4"):
        gpu.ransac_relpose(x, x, {"tangent_sampson": True})


# ------------------------------------------------------------------------------------------ streaming scorer
STREAM_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
import poselib_amd as P
import test_gpu_tangent_sampson as T
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

    chunk = int(_lib.lib().pl_debug_tangent_chunk())
    assert 8 <= chunk <= 512
    return [5, chunk - 1, chunk, chunk + 1, 1000]


def stream_inputs(n):
    d, x1, x2, c1, c2 = GT.scene("RADIAL_FISHEYE", "SIMPLE_RADIAL_FISHEYE", n, 0.0 if n <= 5 else 0.3, 120.0, 9700 + n)
    scale, x1s, x2s, c1s, c2s = GT.scaled_inputs(x1, x2, c1, c2)
    return d, x1s, x2s, c1s, c2s, GT.MAX_ERROR * scale


def stream_models(d, H):
    """the ground truth disturbed at every scale from 1e-5 to 1 (good models keep hundreds of pairs, bad ones a handful), a pose with
    a NaN and t = 0 among them"""
    rs = np.random.RandomState(1000 + H)
    M = np.zeros((H, 7))
    for k in range(H):
        s = 10.0 ** rs.uniform(-5, 0)
        q = np.asarray(d["q_gt"]) + s * rs.randn(4)
        t = np.asarray(d["t_gt"]) + s * rs.randn(3)
        M[k] = np.r_[q / np.linalg.norm(q), t]
    M[0] = np.r_[d["q_gt"], d["t_gt"]]
    if H > 3:
        M[H // 2, 5] = np.nan
        M[H - 2, 4:] = 0.0
    return M


def stream_run(P, n, H):
    d, x1s, x2s, c1s, c2s, thr = stream_inputs(n)
    pr = P.TangentProblem(x1s, x2s, c1s, c2s)
    cnt, sc, path = pr.score_stream(stream_models(d, H), thr)
    pr.close()
    return cnt.copy(), sc.copy(), path


def test_streaming_scorer_equals_the_sequential_scorer_with_and_without_the_filter(gpu):
    """k_score_tangent (fp32 pre-filter, queue, exact drain) against k_score_seq<EST_RELT>: the same counts for 1, 63, 64, 65 and 200
    models on 5, chunk - 1, chunk, chunk + 1 and 1000 correspondences; the scores agree to the rounding of a sum of n terms in
    another order (n 2^-52 of the score: every term is non-negative).  The same runs in a fresh process with
    POSELIB_AMD_NO_PREFILTER=1 (every pair evaluated exactly) give the same bits: the filter only removes work."""
    import os
    import subprocess
    import sys

    got = {}
    filtered = 0
    for n in stream_sizes(gpu):
        d, x1s, x2s, c1s, c2s, thr = stream_inputs(n)
        pr = gpu.TangentProblem(x1s, x2s, c1s, c2s)
        for H in STREAM_MODELS:
            M = stream_models(d, H)
            cnt, sc, path = pr.score_stream(M, thr)
            filtered += path == 1
            for k in range(H):
                s, c = pr.score(gpu.CameraPose(M[k, :4], M[k, 4:]), thr)
                assert cnt[k] == c, (n, H, k, cnt[k], c)
                assert abs(sc[k] - s) <= (n + 64) * 2.0 ** -52 * s, (n, H, k, sc[k], s)
            if H > 3:
                assert cnt[H // 2] == 0 and cnt[H - 2] == 0  # NaN pose, t = 0
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
LOSS = {"truncated": "TRUNCATED", "cauchy": "CAUCHY"}


@pytest.mark.parametrize("n", GT.REFINE_N)
@pytest.mark.parametrize("run", sorted(GT.REFINE_RUNS))
def test_refinement_equals_the_reference(gpu, n, run):
    """Refiner<EST_RELT> in k_lm on the device's own bearings and Jacobians: up to 256 correspondences the sums run in the reference's
    order - pose bit for bit; beyond, identical iteration counts, the pose within 1e-6 (tests/test_gpu_radial_cameras.py) and the
    bits recorded in tests/golden/lm_tree_bits_v1.json"""
    want = G["refine"][f"{n}/{run}"]
    got, it = GT.refine_on_device(gpu, n, run)
    ref = floats(want["pose"])
    print(n, run, "iterations", it, want["iterations"], "max |pose difference|", float(np.abs(got - ref).max()))
    assert it == want["iterations"]
    if n <= 256:
        assert GT.reprs(got) == want["pose"]
    else:
        assert np.abs(got - ref).max() < 1e-6
        LC.assert_pinned("tangent", f"{n}/{run}", got, it)


# ------------------------------------------------------------------------------------------ estimator
def estimate_case(gpu, name):
    case = [c for c in GT.EST_CASES if c[0] == name][0]
    rec = G["estimates"][name]
    d, x1, x2, c1, c2, initial = GT.est_inputs(case, rec["data_seed"])
    assert digest([x1, x2]) == rec["input_sha256"], "the inputs changed: regenerate the fixture"
    null = {"model": -1, "params": []}
    init = None if initial is None else gpu.CameraPose(initial[:4], initial[4:])
    opt = {k: v for k, v in rec["options"].items()}
    pose, info = gpu.estimate_relative_pose(x1, x2, c1 or null, c2 or null, opt, init)
    return rec, pose, info


@pytest.mark.parametrize("name", [c[0] for c in GT.EST_CASES])
def test_estimate_relative_pose_takes_the_references_decisions(gpu, name):
    """every recorded case - fisheye + pinhole and two fisheye cameras at 80 and 150 degrees, OPENCV, identity cameras on calibrated
    points, 30 % and 60 % outliers, PROSAC, a warm start (the identity is what gets scored), n = 5, 6, 7 and 1000: iterations,
    refinements, num_inliers and mask of the reference's run, q and t / |t| within 1e-6 (README.md)"""
    rec, pose, info = estimate_case(gpu, name)
    n = rec["n"]
    mask = np.unpackbits(np.frombuffer(bytes.fromhex(rec["mask_hex"]), dtype=np.uint8))[:n].astype(bool)
    ref = floats(rec["model"])
    q, t = np.asarray(pose.q), np.asarray(pose.t)
    dq = min(np.abs(q - ref[:4]).max(), np.abs(q + ref[:4]).max())
    dt = np.abs(t / np.linalg.norm(t) - ref[4:] / np.linalg.norm(ref[4:])).max()
    print(name, "iterations", info["iterations"], rec["iterations"], "refinements", info["refinements"], rec["refinements"], "inliers",
          info["num_inliers"], rec["num_inliers"], "dq", float(dq), "dt", float(dt))
    assert (info["iterations"], info["refinements"], info["num_inliers"]) == (rec["iterations"], rec["refinements"], rec["num_inliers"])
    assert (np.array(info["inliers"]) == mask).all()
    assert dq < 1e-6 and dt < 1e-6


def test_too_few_points_give_default_stats_and_the_identity(gpu):
    """n < 5 (ransac_impl.h:161-163): the loop does not run"""
    d, x1, x2, c1, c2 = GT.scene("RADIAL_FISHEYE", None, 8, 0.0, 80.0, 9800)
    pose, info = gpu.estimate_relative_pose(x1[:4], x2[:4], c1, c2, {"max_error": GT.MAX_ERROR, "tangent_sampson": True})
    assert (info["iterations"], info["refinements"], info["num_inliers"]) == (0, 0, 0)
    assert np.r_[pose.q, pose.t].tolist() == [1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    assert not any(info["inliers"])


# ------------------------------------------------------------------------------------------ batch
def test_batch_items_with_the_flag_run_solo_and_equal_their_single_calls(gpu):
    """8 tangent items mixed with 8 plain relative-pose and 8 absolute-pose items: every result equals the single call bit for bit,
    and the report counts the tangent items under `solo`"""
    problems, singles = [], []
    for k in range(8):
        d, x1, x2, c1, c2 = GT.scene("RADIAL_FISHEYE", "SIMPLE_RADIAL_FISHEYE", 300 + 7 * k, 0.3, 120.0, 9900 + k)
        ot = {"max_error": GT.MAX_ERROR, "tangent_sampson": True, "ransac": {"seed": k}}
        op = {"max_error": GT.MAX_ERROR, "ransac": {"seed": k}}
        problems += [("rel", x1, x2, c1, c2, ot), ("rel", x1, x2, c1, c2, op)]
        singles += [gpu.estimate_relative_pose(x1, x2, c1, c2, ot), gpu.estimate_relative_pose(x1, x2, c1, c2, op)]
        a = synth.absolute_pose_scene(400 + 5 * k, 0.3, 9950 + k)
        oa = {"max_error": 2.0, "ransac": {"seed": k}}
        problems.append(("abs", a["p2d"], a["p3d"], a["camera"], oa))
        img, info = gpu.estimate_absolute_pose(a["p2d"], a["p3d"], a["camera"], oa)
        singles.append((img.pose, info))
    out = gpu.estimate_batch(problems)
    report = gpu.last_batch_report()
    print(report)
    assert report["items"] == 24 and report["solo"] == 8
    for k, ((m, info), (m1, info1)) in enumerate(zip(out, singles)):
        pose = m.pose if hasattr(m, "pose") else m
        assert GT.reprs(np.r_[pose.q, pose.t]) == GT.reprs(np.r_[m1.q, m1.t]), k
        for key in ("iterations", "refinements", "num_inliers", "inliers"):
            assert info[key] == info1[key], (k, key)
        assert repr(info["model_score"]) == repr(info1["model_score"]), k


# ------------------------------------------------------------------------------------------ rejections
@pytest.mark.parametrize("flag", ["refine_focal_length", "refine_principal_point", "refine_extra_params"])
def test_refined_intrinsics_with_the_flag_are_unsupported(gpu, flag):
    d, x1, x2, c1, c2 = GT.scene("RADIAL_FISHEYE", None, 50, 0.0, 80.0, 9801)
    with pytest.raises(gpu.PoseLibAmdError, match="error -4.*fixed cameras"):
        gpu.estimate_relative_pose(x1, x2, c1, c2, {"tangent_sampson": True, "bundle": {flag: True}})
