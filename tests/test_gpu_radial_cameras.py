"""GPU parity (-m gpu) of the SIMPLE_RADIAL and RADIAL camera models through the C-ABI / poselib_amd, against
tests/golden/golden_cameras_v1.json - outputs of the reference's own sources, recorded on the CPU by
tests/golden/make_golden_cameras.py (the reference build is not available next to a GPU, and the oracle's restatement does not know
these models: nothing here calls it with them).

Standards, the project's existing ones: un-projection and bundle adjustment of up to 256 correspondences bit for bit
(test_gpu_intrinsics.py), identical LM iteration counts beyond; the estimators take every decision of the recorded reference run -
iterations, refinements, num_inliers, mask - and return the model within 1e-6 (README.md), the relative pose with t normalised.
"""
import json

import numpy as np
import pytest

from golden import make_golden_cameras as GC
from golden.make_golden import digest
from poselib_amd import synth

pytestmark = pytest.mark.gpu

G = json.load(open(GC.PATH))
MODELS = sorted(GC.MODELS)


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
    cam, pix = GC.unproject_inputs(model)[name]
    want = G[model]["unproject"][name]
    assert digest([pix]) == want["input_sha256"], "the inputs changed: regenerate the fixture"
    got = gpu.undistort_points(GC.named(cam), pix)
    head = GC.undistorted_pixels(cam, floats(want["head"]).reshape(-1, 2))
    k = len(head)
    print(model, name, "max |difference| over the first", k, "points:", float(np.abs(got[:k] - head).max()))
    assert GC.reprs(got[:k]) == GC.reprs(head)
    assert digest([got]) == want["undistorted_sha256"]


# ------------------------------------------------------------------------------------------ bundle adjustment
def _bundle_case(gpu, model, n):
    pix, X, gt, cam0, p0 = GC.bundle_inputs(model, n)
    rec = G[model]["bundle"]
    assert digest([pix, X, p0, cam0["params"]]) == rec[f"{n}/input_sha256"], "the inputs changed: regenerate the fixture"
    return pix, X, gt, GC.named(cam0), p0, rec, gpu.Problem(gpu.KIND_ABS, pix, X)


def _run_bundle(gpu, pr, key, bo, cam0, p0, mask):
    start = gpu.CameraPose(p0[:4], p0[4:])
    if key.startswith("pose"):
        pose, it = pr.refine(start, bo, camera=cam0, mask=mask)
        return pose7(pose), np.asarray(cam0["params"]), it
    pose, cam, it = pr.bundle_adjust(start, cam0, bo, mask=mask)
    return pose7(pose), np.asarray(cam.params), it


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("n", GC.SMALL_N)
def test_bundle_adjust_and_refine_bit_exact_up_to_256_correspondences(gpu, model, n):
    """Problem.refine with the camera (k_lm) and Problem.bundle_adjust with the five flag sets (k_lm_cam), CAUCHY and HUBER"""
    pix, X, gt, cam0, p0, rec, pr = _bundle_case(gpu, model, n)
    runs = GC.bundle_runs(n)
    assert len(runs) == 12
    for key, bo, _ in runs:
        want = rec[f"{n}/{key}"]
        pose, cam, it = _run_bundle(gpu, pr, key, bo, cam0, p0, None)
        print(model, n, key, "iterations", it, want["iterations"], "max |pose difference|", float(np.abs(pose - floats(want["pose"])).max()),
              "max |camera difference|", float(np.abs(cam - floats(want["camera"])).max()))
        assert it == want["iterations"], (model, n, key, it, want["iterations"])
        assert GC.reprs(pose) == want["pose"], (model, n, key)
        assert GC.reprs(cam) == want["camera"], (model, n, key)
    pr.close()


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("n", GC.LARGE_N)
def test_bundle_adjust_and_refine_larger_problems_with_and_without_mask(gpu, model, n):
    """identical iteration counts; the result within 1e-6 of the recorded one (the project's contract for a model)"""
    pix, X, gt, cam0, p0, rec, pr = _bundle_case(gpu, model, n)
    runs = GC.bundle_runs(n)
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
@pytest.mark.parametrize("name", [c[0] for c in GC.ABS_CASES])
def test_estimate_absolute_pose_matches_the_recorded_reference_run(gpu, model, name):
    """n = 1500 (the matrix-core pre-filter is on the path) and 400, 30 % and 60 % outliers; plain, with estimate_focal_length,
    with bundle.refine_*"""
    _, n, outl, opt, start = next(c for c in GC.ABS_CASES if c[0] == name)
    c = G[model]["estimators"][name]
    d, pix, cam_in = GC.abs_inputs(model, n, outl, start, c["data_seed"])
    assert digest([pix, d["p3d"]]) == c["input_sha256"], "the inputs changed: regenerate the fixture"
    img, info = gpu.estimate_absolute_pose(pix, d["p3d"], GC.named(cam_in), c["options"])
    _assert_decisions(info, c, (model, name))
    assert int(unpack_mask(c).sum()) == int(d["inlier_gt"].sum())  # (a successful match was recorded)
    want_cam = floats(c["camera"])
    dp = float(np.abs(pose7(img.pose) - floats(c["model"])).max())
    dc = float(np.abs(np.asarray(img.camera.params) - want_cam).max())
    print(model, name, "max |pose difference|", dp, "max |camera difference|", dc)
    assert dp < 1e-6
    assert dc < 1e-6 * max(1.0, np.abs(want_cam).max())
    if start is not None:  # the focal length was estimated or refined: it moved towards the truth
        assert abs(img.camera.params[0] - GC.F) < abs(cam_in["params"][0] - GC.F)


@pytest.mark.parametrize("name", [c[0] for c in GC.REL_CASES])
def test_estimate_relative_pose_matches_the_recorded_reference_run(gpu, name):
    """one radial and one pinhole camera; two radial cameras"""
    _, m1, m2, n, outl = next(c for c in GC.REL_CASES if c[0] == name)
    c = G["relative"][name]
    d, x1, x2, c1, c2 = GC.rel_inputs(m1, m2, n, outl, c["data_seed"])
    assert digest([x1, x2]) == c["input_sha256"], "the inputs changed: regenerate the fixture"
    pose, info = gpu.estimate_relative_pose(x1, x2, GC.named(c1), c2 if m2 is None else GC.named(c2), c["options"])
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
    for k in range(12):
        for model in MODELS:
            d, pix, cam_in = GC.abs_inputs(model, 300 + 40 * k, 0.3 + 0.02 * k, None, 7800 + k)
            probs.append(("abs", pix, d["p3d"], GC.named(cam_in), {"max_error": 4.0, "ransac": {"seed": k}}))
        d, pix, cam_in = GC.abs_inputs("RADIAL", 1200, 0.4, (0.002, 1.0), 7820 + k)
        probs.append(("abs", pix, d["p3d"], GC.named(cam_in), {"max_error": 8.0, "ransac": {"seed": k}, "bundle": dict(GC.FLAGS[4])}))
        d = synth.absolute_pose_scene(500, 0.4, 7840 + k)
        probs.append(("abs", d["p2d"], d["p3d"], d["camera"], {"ransac": {"seed": k}}))
        d, x1, x2, c1, c2 = GC.rel_inputs("SIMPLE_RADIAL", "RADIAL" if k % 2 else None, 400 + 30 * k, 0.3, 7860 + k)
        probs.append(("rel", x1, x2, GC.named(c1), GC.named(c2) if k % 2 else c2, {"max_error": GC.REL_MAX_ERROR, "ransac": {"seed": k}}))
        d = synth.relative_pose_scene(400, 0.3, 7880 + k)
        probs.append(("rel", d["x1"], d["x2"], d["camera1"], d["camera2"], {"ransac": {"seed": k}}))
    return probs


def test_mixed_batch_with_radial_cameras_equals_the_single_calls_and_runs_in_groups(gpu):
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
def test_prefilter_bound_covers_strong_barrel_distortion(gpu):
    """The scorers' fp32 / fp16 pre-filters are conservative only under a bound of max(|x|, |y|) of the UN-PROJECTED points.  Under
    strong barrel distortion (k1 = -0.2, field of view 80 degrees: 39 % at the image corners) these lie far outside (pixel - c) / f, which is all a host pass
    over the pixels could know: the front-end must read the bound back from the device.  Every count of the streaming scorer equals
    the exact scorer's, and the front-end keeps every inlier."""
    rs = np.random.RandomState(91)
    for model, extra in (("SIMPLE_RADIAL", [-0.2]), ("RADIAL", [-0.2, 0.01])):
        d = synth.absolute_pose_scene(4000, 0.5, 7900 + GC.MODELS[model], fov_deg=80.0)
        cam = GC.camera(model, extra)
        pix = synth.radial_distort_pixels(np.asarray(d["p2d"]), cam["params"])
        lin = np.abs((pix - [GC.CX, GC.CY]) / GC.F).max()
        un = (gpu.undistort_points(GC.named(cam), pix) - [GC.CX, GC.CY]) / GC.F
        inl = d["inlier_gt"]
        print(model, "max |(pixel - c) / f|", float(lin), "max |un-projected|", float(np.abs(un[inl]).max()))
        assert np.abs(un[inl]).max() > 1.1 * np.abs(((pix - [GC.CX, GC.CY]) / GC.F)[inl]).max()  # well above the linear bound
        assert np.abs(un[inl] - (np.asarray(d["p2d"])[inl] - [GC.CX, GC.CY]) / GC.F).max() < 1e-6  # (the inverse did converge)
        # the streaming scorer on the un-projected points: models around the truth, thresholds on both filter paths
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
            assert cnt[0] >= 0.99 * inl.sum()  # (the ground truth itself: the noise is 0.0005)
        pr.close()
        # ... and through the front-end, whose bound comes from k_prepare: every ground-truth inlier is found
        img, info = gpu.estimate_absolute_pose(pix, d["p3d"], GC.named(cam), {"max_error": 4.0, "ransac": {"seed": 5}})
        mask = np.asarray(info["inliers"], dtype=bool)
        print(model, "front-end inliers", int(mask.sum()), "of", int(inl.sum()))
        assert mask[inl].all() and int((mask & ~inl).sum()) <= 2


# ------------------------------------------------------------------------------------------ malformed cameras
def test_malformed_cameras_raise_and_do_not_fault(gpu):
    d = synth.absolute_pose_scene(100, 0.2, 7950)
    r = synth.relative_pose_scene(100, 0.2, 7951)
    bad = [{"model": mid, "params": [1000.0, 500.0, 500.0] + [0.0] * 9} for mid in range(5, 12)]
    bad.append({"model": "RADIAL", "params": [1000.0, 500.0, 500.0, -0.1]})
    bad.append({"model": "SIMPLE_RADIAL", "params": [1000.0, 500.0, 500.0]})
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
    cam = GC.named(GC.camera("RADIAL"))
    pix = synth.radial_distort_pixels(np.asarray(d["p2d"]), cam["params"])
    img, info = gpu.estimate_absolute_pose(pix, d["p3d"], cam, {"max_error": 4.0})
    assert info["num_inliers"] == int(d["inlier_gt"].sum())
