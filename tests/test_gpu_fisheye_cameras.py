"""GPU parity (-m gpu) of the OPENCV_FISHEYE, SIMPLE_RADIAL_FISHEYE and RADIAL_FISHEYE camera models through the C-ABI /
poselib_amd, against tests/golden/golden_fisheye_v1.json - outputs of the reference's own sources, recorded on the CPU by
tests/golden/make_golden_fisheye.py (the reference build is not available next to a GPU, and the oracle's restatement does not know
these models: nothing here calls it with them).

Standards, the project's existing ones (tests/test_gpu_radial_cameras.py): un-projection and bundle adjustment of up to 256
correspondences bit for bit, identical LM iteration counts beyond and the model within 1e-6; the estimators take every decision of
the recorded reference run - iterations, refinements, num_inliers, mask - and return the model within 1e-6 (README.md), the relative
pose with t normalised.
"""
import json

import numpy as np
import pytest

from golden import make_golden_fisheye as GF
from golden.make_golden import digest
from poselib_amd import synth

pytestmark = pytest.mark.gpu

G = json.load(open(GF.PATH))
MODELS = sorted(GF.MODELS)


def floats(v):
    return np.array([float(x) for x in v])


def unpack_mask(c):
    return np.unpackbits(np.frombuffer(bytes.fromhex(c["mask_hex"]), dtype=np.uint8))[: c["n"]].astype(bool)


def pose7(p):
    return np.r_[p.q, p.t]


# ------------------------------------------------------------------------------------------ un-projection
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("name", ["disc", "centre", "k0"])
def test_undistort_points_equals_the_recorded_unprojection(gpu, model, name):
    cam, pix = GF.unproject_inputs(model)[name]
    want = G[model]["unproject"][name]
    assert digest([pix]) == want["input_sha256"], "the inputs changed: regenerate the fixture"
    got = gpu.undistort_points(GF.named(cam), pix)
    head = GF.undistorted_pixels(cam, floats(want["head"]).reshape(-1, 2))
    k = len(head)
    print(model, name, "max |difference| over the first", k, "points:", float(np.abs(got[:k] - head).max()))
    assert GF.reprs(got[:k]) == GF.reprs(head)
    assert digest([got]) == want["undistorted_sha256"]


# ------------------------------------------------------------------------------------------ bundle adjustment
def _bundle_case(gpu, model, n):
    pix, X, gt, cam0, p0 = GF.bundle_inputs(model, n)
    rec = G[model]["bundle"]
    assert digest([pix, X, p0, cam0["params"]]) == rec[f"{n}/input_sha256"], "the inputs changed: regenerate the fixture"
    return pix, X, gt, GF.named(cam0), p0, rec, gpu.Problem(gpu.KIND_ABS, pix, X)


def _run_bundle(gpu, pr, key, bo, cam0, p0, mask):
    start = gpu.CameraPose(p0[:4], p0[4:])
    if key.startswith("pose"):
        pose, it = pr.refine(start, bo, camera=cam0, mask=mask)
        return pose7(pose), np.asarray(cam0["params"]), it
    pose, cam, it = pr.bundle_adjust(start, cam0, bo, mask=mask)
    return pose7(pose), np.asarray(cam.params), it


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("n", GF.SMALL_N)
def test_bundle_adjust_and_refine_bit_exact_up_to_256_correspondences(gpu, model, n):
    """Problem.refine with the camera (k_lm) and Problem.bundle_adjust with the five flag sets (k_lm_cam), CAUCHY and HUBER"""
    pix, X, gt, cam0, p0, rec, pr = _bundle_case(gpu, model, n)
    runs = GF.bundle_runs(n)
    assert len(runs) == 12
    for key, bo, _ in runs:
        want = rec[f"{n}/{key}"]
        pose, cam, it = _run_bundle(gpu, pr, key, bo, cam0, p0, None)
        print(model, n, key, "iterations", it, want["iterations"], "max |pose difference|", float(np.abs(pose - floats(want["pose"])).max()),
              "max |camera difference|", float(np.abs(cam - floats(want["camera"])).max()))
        assert it == want["iterations"], (model, n, key, it, want["iterations"])
        assert GF.reprs(pose) == want["pose"], (model, n, key)
        assert GF.reprs(cam) == want["camera"], (model, n, key)
    pr.close()


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("n", GF.LARGE_N)
def test_bundle_adjust_and_refine_larger_problems_with_and_without_mask(gpu, model, n):
    """identical iteration counts; the result within 1e-6 of the recorded one (the project's contract for a model)"""
    pix, X, gt, cam0, p0, rec, pr = _bundle_case(gpu, model, n)
    runs = GF.bundle_runs(n)
    assert len(runs) == 6 and {m for _, _, m in runs} == {True, False}
    for key, bo, masked in runs:
        want = rec[f"{n}/{key}"]
        pose, cam, it = _run_bundle(gpu, pr, key, bo, cam0, p0, gt if masked else None)
        dp, dc = float(np.abs(pose - floats(want["pose"])).max()), float(np.abs(cam - floats(want["camera"])).max())
        print(model, n, key, "iterations", it, want["iterations"], "max |pose difference|", dp, "max |camera difference|", dc)
        assert it == want["iterations"], (model, n, key, it, want["iterations"])
        assert dp < 1e-6 and dc < 1e-6 * max(1.0, np.abs(floats(want["camera"])).max()), (model, n, key, dp, dc)
    pr.close()


# ------------------------------------------------------------------------------------------ estimators
def _assert_decisions(info, c, tag):
    print(tag, {k: (info[k], c[k]) for k in ("iterations", "refinements", "num_inliers")})
    for k in ("iterations", "refinements", "num_inliers"):
        assert info[k] == c[k], (tag, k, info[k], c[k])
    assert np.array_equal(np.asarray(info["inliers"], dtype=bool), unpack_mask(c)), tag


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("name", [c[0] for c in GF.ABS_CASES])
def test_estimate_absolute_pose_matches_the_recorded_reference_run(gpu, model, name):
    """80 and 150 degrees field of view, n = 200 .. 3000 (from 1024 on the matrix-core pre-filter is on the path), 30 % and 50 %
    outliers; plain, with estimate_focal_length, with bundle.refine_*.  The 150-degree scenes: masks and scores equal the
    reference's."""
    _, n, outl, fov, opt, start = next(c for c in GF.ABS_CASES if c[0] == name)
    c = G[model]["estimators"][name]
    d, pix, cam_in = GF.abs_inputs(model, n, outl, fov, start, c["data_seed"])
    assert digest([pix, d["p3d"]]) == c["input_sha256"], "the inputs changed: regenerate the fixture"
    img, info = gpu.estimate_absolute_pose(pix, d["p3d"], GF.named(cam_in), c["options"])
    _assert_decisions(info, c, (model, name))
    assert int(unpack_mask(c).sum()) == int(d["inlier_gt"].sum())  # (a successful match was recorded)
    want_cam = floats(c["camera"])
    dp = float(np.abs(pose7(img.pose) - floats(c["model"])).max())
    dc = float(np.abs(np.asarray(img.camera.params) - want_cam).max())
    ds = abs(info["model_score"] - float(c["model_score"]))
    print(model, name, "max |pose difference|", dp, "max |camera difference|", dc, "|score difference|", ds)
    assert dp < 1e-6
    assert dc < 1e-6 * max(1.0, np.abs(want_cam).max())
    assert ds <= 1e-9 * abs(float(c["model_score"]))  # (the score: a sum over the same mask of the same residuals)
    if start is not None:  # the focal length was estimated or refined: it moved towards the truth
        assert abs(img.camera.params[0] - GF.F) < abs(cam_in["params"][0] - GF.F)


@pytest.mark.parametrize("name", [c[0] for c in GF.REL_CASES])
def test_estimate_relative_pose_matches_the_recorded_reference_run(gpu, name):
    """one fisheye and one pinhole camera; two fisheye cameras, up to 120 degrees field of view"""
    _, m1, m2, n, outl, fov = next(c for c in GF.REL_CASES if c[0] == name)
    c = G["relative"][name]
    d, x1, x2, c1, c2 = GF.rel_inputs(m1, m2, n, outl, fov, c["data_seed"])
    assert digest([x1, x2]) == c["input_sha256"], "the inputs changed: regenerate the fixture"
    pose, info = gpu.estimate_relative_pose(x1, x2, GF.named(c1), c2 if m2 is None else GF.named(c2), c["options"])
    _assert_decisions(info, c, name)
    want = floats(c["model"])
    got = pose7(pose)
    dq = float(np.abs(got[:4] - want[:4]).max())
    dt = float(np.abs(got[4:] / np.linalg.norm(got[4:]) - want[4:] / np.linalg.norm(want[4:])).max())
    print(name, "max |q difference|", dq, "max |t / |t| difference|", dt)
    assert dq < 1e-6 and dt < 1e-6


# ------------------------------------------------------------------------------------------ batches
def _batch_problems():
    probs = []
    for k in range(10):
        for model in MODELS:
            d, pix, cam_in = GF.abs_inputs(model, 300 + 40 * k, 0.3 + 0.02 * k, 80.0 if k % 2 else 150.0, None, 8800 + k)
            probs.append(("abs", pix, d["p3d"], GF.named(cam_in), {"max_error": 2.0, "ransac": {"seed": k}}))
        d, pix, cam_in = GF.abs_inputs("OPENCV_FISHEYE", 1200, 0.4, 80.0, (0.002, 1.0), 8820 + k)
        probs.append(("abs", pix, d["p3d"], GF.named(cam_in), {"max_error": 8.0, "ransac": {"seed": k}, "bundle": dict(GF.FLAGS[4])}))
        d = synth.absolute_pose_scene(500, 0.4, 8840 + k)
        probs.append(("abs", d["p2d"], d["p3d"], d["camera"], {"ransac": {"seed": k}}))
        d, x1, x2, c1, c2 = GF.rel_inputs("SIMPLE_RADIAL_FISHEYE", "OPENCV_FISHEYE" if k % 2 else None, 400 + 30 * k, 0.3, 80.0, 8860 + k)
        probs.append(("rel", x1, x2, GF.named(c1), GF.named(c2) if k % 2 else c2, {"max_error": GF.REL_MAX_ERROR, "ransac": {"seed": k}}))
        d = synth.relative_pose_scene(400, 0.3, 8880 + k)
        probs.append(("rel", d["x1"], d["x2"], d["camera1"], d["camera2"], {"ransac": {"seed": k}}))
    return probs


def test_mixed_batch_with_fisheye_cameras_equals_the_single_calls_and_runs_in_groups(gpu):
    probs = _batch_problems()
    assert len(probs) >= 64
    singles = []
    for pr in probs:
        if pr[0] == "abs":
            singles.append(gpu.estimate_absolute_pose(pr[1], pr[2], pr[3], pr[4]))
        else:
            singles.append(gpu.estimate_relative_pose(pr[1], pr[2], pr[3], pr[4], pr[5]))
    res = gpu.estimate_batch(probs, max_in_flight=4)
    report = gpu.last_batch_report()
    print("batch report", report)
    assert report["items"] == len(probs) and report["solo"] == 0, report
    for i, (pr, got, want) in enumerate(zip(probs, res, singles)):
        if pr[0] == "abs":
            (img, info), (simg, sinfo) = got, want
            assert np.array_equal(pose7(img.pose), pose7(simg.pose)), i
            assert np.array_equal(img.camera.params, simg.camera.params), i
        else:
            (pose, info), (spose, sinfo) = got, want
            assert np.array_equal(pose7(pose), pose7(spose)), i
        for k in ("iterations", "refinements", "num_inliers", "inliers"):
            assert info[k] == sinfo[k], (i, k)
        assert info["num_inliers"] > 0.3 * len(pr[1]), i


# ------------------------------------------------------------------------------------------ the pre-filter bound
def test_prefilter_bound_covers_a_150_degree_field_of_view(gpu):
    """The un-projected points of a 150-degree scene reach |x| = tan(75 degrees) = 3.7, where (pixel - c) / f stays below 1.4: the
    bound of the matrix-core pre-filter must come from the device.  Every ground-truth inlier is kept by the front-end, and the
    streaming scorer's counts on the un-projected points equal the exact scorer's."""
    rs = np.random.RandomState(93)
    for model in MODELS:
        d, pix, cam = GF.abs_inputs(model, 3000, 0.5, GF.WIDE_FOV_DEG, None, 8900 + GF.MODELS[model])
        fx, fy, cx, cy, _ = GF.layout(cam)
        un = (gpu.undistort_points(GF.named(cam), pix) - [cx, cy]) / [fx, fy]
        inl = d["inlier_gt"]
        lin = np.abs((pix - [cx, cy]) / [fx, fy])[inl].max()
        print(model, "max |(pixel - c) / f|", float(lin), "max |un-projected|", float(np.abs(un[inl]).max()))
        assert np.abs(un[inl]).max() > 2.0 * lin
        assert np.abs(un[inl] - (np.asarray(d["p2d"])[inl] - [GF.CX, GF.CY]) / GF.F).max() < 1e-6  # (the inverse did converge)
        M = [np.r_[d["q_gt"], d["t_gt"]]]
        for _ in range(7):
            q = d["q_gt"] + 0.01 * rs.randn(4)
            M.append(np.r_[q / np.linalg.norm(q), d["t_gt"] + 0.02 * rs.randn(3)])
        M = np.array(M)
        pr = gpu.Problem(gpu.KIND_ABS, un, d["p3d"])
        for thr in (0.004, 0.012, 0.5):
            cnt, sc, path = pr.score_stream(M, thr)
            assert path == 2, (model, thr, path)  # the matrix-core filter is on the path
            for k in range(len(M)):
                osc, ocnt = pr.score(gpu.CameraPose(M[k, :4], M[k, 4:]), thr)
                assert cnt[k] == ocnt, (model, thr, k, cnt[k], ocnt)
                assert abs(sc[k] - osc) <= 1e-9 * abs(osc) + 1e-300
        pr.close()
        img, info = gpu.estimate_absolute_pose(pix, d["p3d"], GF.named(cam), {"max_error": 2.0, "ransac": {"seed": 5}})
        mask = np.asarray(info["inliers"], dtype=bool)
        print(model, "front-end inliers", int(mask.sum()), "of", int(inl.sum()))
        assert int((~mask & inl).sum()) <= 1 and int((mask & ~inl).sum()) <= 2  # (0.5 px noise at max_error 2.0: one in 3000 may fall out)


# ------------------------------------------------------------------------------------------ malformed cameras
def test_cameras_with_too_few_or_too_many_parameters_raise_and_do_not_fault(gpu):
    """a fisheye camera carries exactly its model's parameters: the reference's un-projection would read a ninth (fifth, sixth) one
    as a further coefficient, which its projection does not know"""
    d = synth.absolute_pose_scene(100, 0.2, 8950)
    r = synth.relative_pose_scene(100, 0.2, 8951)
    bad = [{"model": "OPENCV_FISHEYE", "params": [1000.0, 1000.0, 500.0, 500.0, 0.0, 0.0, 0.0]},
           {"model": "OPENCV_FISHEYE", "params": [1000.0, 500.0, 500.0]},
           {"model": "SIMPLE_RADIAL_FISHEYE", "params": [1000.0, 500.0, 500.0]},
           {"model": "RADIAL_FISHEYE", "params": [1000.0, 500.0, 500.0, -0.03]},
           {"model": "RADIAL_FISHEYE", "params": []},
           {"model": "OPENCV_FISHEYE", "params": [1000.0, 1000.0, 500.0, 500.0, 0.0, 0.0, 0.0, 0.0, 0.01]},
           {"model": "SIMPLE_RADIAL_FISHEYE", "params": [1000.0, 500.0, 500.0, -0.03, 0.004]},
           {"model": "RADIAL_FISHEYE", "params": [1000.0, 500.0, 500.0, -0.03, 0.004, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]}]
    bad += [{"model": mid, "params": [1000.0, 500.0, 500.0] + [0.0] * 9} for mid in (6, 7, 10, 11, 12, 13)]  # still out of scope
    pr = gpu.Problem(gpu.KIND_ABS, d["p2d"], d["p3d"])
    start = gpu.CameraPose(d["q_gt"], d["t_gt"])
    for cam in bad:
        with pytest.raises(gpu.PoseLibAmdError):
            gpu.estimate_absolute_pose(d["p2d"], d["p3d"], cam, {})
        with pytest.raises(gpu.PoseLibAmdError):
            gpu.estimate_relative_pose(r["x1"], r["x2"], cam, r["camera2"], {})
        with pytest.raises(gpu.PoseLibAmdError):
            gpu.estimate_relative_pose(r["x1"], r["x2"], r["camera1"], cam, {})
        with pytest.raises(gpu.PoseLibAmdError):
            gpu.undistort_points(cam, d["p2d"])
        with pytest.raises(gpu.PoseLibAmdError):
            pr.bundle_adjust(start, cam, {"refine_focal_length": True})
        with pytest.raises(gpu.PoseLibAmdError):
            pr.refine(start, {}, camera=cam)
    pr.close()
    # the library still works afterwards
    cam = GF.camera("RADIAL_FISHEYE")
    img, info = gpu.estimate_absolute_pose(GF.through(cam, np.asarray(d["p2d"])), d["p3d"], GF.named(cam), {"max_error": 4.0})
    assert info["num_inliers"] == int(d["inlier_gt"].sum())
