"""OPENCV_FISHEYE, SIMPLE_RADIAL_FISHEYE and RADIAL_FISHEYE cameras on the CPU: the device math headers (pl_libm.h, pl_refine.h,
pl_refine_cam.h) compiled for the host (tests/hostmath) against the reference's own camera models and bundle adjustment, bit for bit.

The comparator is tests/golden/golden_fisheye_v1.json, recorded from the reference build (oracle/_ref) by
tests/golden/make_golden_fisheye.py; where that build is present the fixture is also held to it, entry for entry.  The oracle's
restatement (liboracle.so) does not know these models and is never called with them here.

A library without the three models sends them through the NULL-camera branch of every switch: these tests then fail.
"""
import json

import numpy as np
import pytest

import hostmath_lib as HM
import ref_lib
from golden import make_golden_fisheye as GF
from golden.make_golden import digest

G = json.load(open(GF.PATH))
LOSS_IDS = {"TRIVIAL": 0, "TRUNCATED": 1, "HUBER": 2, "CAUCHY": 3}
EXTRA_IDX = {"OPENCV_FISHEYE": ([0, 1], [2, 3], [4, 5, 6, 7]), "SIMPLE_RADIAL_FISHEYE": ([0], [1, 2], [3]), "RADIAL_FISHEYE": ([0], [1, 2], [3, 4])}


def hm_camera(cam):
    return HM.camera_params(cam["model"], cam["params"])


def flag_bits(bo):
    return (1 if bo.get("refine_focal_length") else 0) | (2 if bo.get("refine_principal_point") else 0) | (4 if bo.get("refine_extra_params") else 0)


def hm_options(bo):
    return HM.lm_options(bo.get("max_iterations", 100), LOSS_IDS[bo["loss_type"]], bo["loss_scale"])


@pytest.mark.parametrize("model", sorted(GF.MODELS))
@pytest.mark.parametrize("name", ["disc", "centre", "k0"])
def test_unproject_equals_the_reference_bit_for_bit(model, name):
    """10 000 pixels of rays up to 75 degrees from the axis, the principal point, rings within 1e-9 .. 1e-7 of it on either side of
    rd = 1e-8, all-zero distortion"""
    cam, pix = GF.unproject_inputs(model)[name]
    want = G[model]["unproject"][name]
    assert digest([pix]) == want["input_sha256"], "the inputs changed: regenerate the fixture"
    assert len(pix) == {"disc": 10000, "centre": 41, "k0": 2000}[name]
    got = HM.unproject(hm_camera(cam), pix)
    assert GF.reprs(got[:48]) == want["head"]
    assert digest([got]) == want["sha256"]
    assert digest([GF.undistorted_pixels(cam, got)]) == want["undistorted_sha256"]
    fx, fy, cx, cy, _ = GF.layout(cam)
    if name == "centre":
        assert got[0].tolist() == [0.0, 0.0]
        rd = np.hypot((pix[:, 0] - cx) / fx, (pix[:, 1] - cy) / fy)
        assert (rd <= 1e-8).sum() >= 15 and (rd > 1e-8).sum() >= 15  # both sides of the reference's test
    if name == "disc":  # ... and it is the inverse of the distortion, out to 75 degrees
        from poselib_amd import synth

        back = synth.fisheye_distort_pixels(GF.undistorted_pixels(cam, got), model, cam["params"])
        assert np.abs(back - pix).max() < 1e-6
        assert np.degrees(np.arctan(np.hypot(got[:, 0], got[:, 1]).max())) > 74.0
        assert np.abs(got - np.stack([(pix[:, 0] - cx) / fx, (pix[:, 1] - cy) / fy], axis=1)).max() > 1.0  # (far from a linear camera)


@pytest.mark.parametrize("model", sorted(GF.MODELS))
@pytest.mark.parametrize("n", GF.SMALL_N + GF.LARGE_N)
def test_bundle_adjustment_equals_the_reference_bit_for_bit(model, n):
    """hm_lm with a camera (the pose alone) and hm_lm_cam (intrinsics with the pose): pose, camera parameters and iteration count.
    Up to 256 correspondences: the five flag sets, CAUCHY and HUBER; beyond: with and without a mask.  The serial host statement
    sums in the reference's order at every n, so the larger problems are bit for bit here as well."""
    pix, X, gt, cam0, p0 = GF.bundle_inputs(model, n)
    rec = G[model]["bundle"]
    assert digest([pix, X, p0, cam0["params"]]) == rec[f"{n}/input_sha256"], "the inputs changed: regenerate the fixture"
    cols = [pix[:, 0], pix[:, 1], X[:, 0], X[:, 1], X[:, 2]]
    runs = GF.bundle_runs(n)
    assert len(runs) == (12 if n <= 256 else 6)
    for key, bo, masked in runs:
        want = rec[f"{n}/{key}"]
        mask = gt if masked else None
        if key.startswith("pose"):
            got, it, _ = HM.lm("abs", cols, p0, hm_options(bo), hm_camera(cam0), mask=mask)
            cam = cam0["params"]
        else:
            got, cam, it, costs = HM.lm_cam(cols, p0, hm_options(bo), hm_camera(cam0), flag_bits(bo), mask=mask)
            assert [repr(float(v)) for v in costs] == [want["initial_cost"], want["cost"]], (model, n, key)
            assert GF.reprs(cam) != GF.reprs(cam0["params"])  # the camera did move
        assert it == want["iterations"], (model, n, key, it, want["iterations"])
        assert GF.reprs(got[:7]) == want["pose"], (model, n, key)
        assert GF.reprs(cam) == want["camera"], (model, n, key)
        assert it >= 2


@pytest.mark.parametrize("model", sorted(GF.MODELS))
def test_refinement_indices_follow_the_reference_order(model):
    """get_param_refinement_idx: focal, principal point, extra - seen through which parameters a run moves"""
    focal, pp, extra = EXTRA_IDX[model]
    pix, X, gt, cam0, p0 = GF.bundle_inputs(model, 64)
    cols = [pix[:, 0], pix[:, 1], X[:, 0], X[:, 1], X[:, 2]]
    for flags, moved in ((1, focal), (2, pp), (4, extra), (7, focal + pp + extra)):
        _, cam, _, _ = HM.lm_cam(cols, p0, HM.lm_options(20, 3, 1.0), hm_camera(cam0), flags)
        assert [i for i in range(len(cam)) if cam[i] != cam0["params"][i]] == moved, (model, flags)


@pytest.mark.skipif(not ref_lib.available(), reason="oracle/_ref not built and the reference sources absent")
@pytest.mark.parametrize("part", ["unproject", "bundle"])
def test_fixture_equals_the_live_reference(part):
    live = GF.record(parts=(part,))
    for model in GF.MODELS:
        assert live[model][part] == G[model][part], (model, part)


@pytest.mark.skipif(not ref_lib.available(), reason="oracle/_ref not built and the reference sources absent")
def test_fixture_estimator_runs_equal_the_live_reference_and_are_successful_matches():
    """every recorded RANSAC run again, with its recorded seeds: same decisions, same model bit for bit - and a match that found the
    ground truth (the generator's own condition)"""
    with ref_lib.reference() as R:
        for model in GF.MODELS:
            for name, n, outl, fov, opt, start in GF.ABS_CASES:
                c = G[model]["estimators"][name]
                d, pix, cam_in = GF.abs_inputs(model, n, outl, fov, start, c["data_seed"])
                assert digest([pix, d["p3d"]]) == c["input_sha256"]
                pose, mask, st, cam_out = R.estimate_absolute_pose(pix, d["p3d"], cam_in, c["options"], return_camera=True)
                assert GF.check_abs_run(d, pose, mask, cam_out), (model, name)
                assert (st["iterations"], st["refinements"], st["num_inliers"]) == (c["iterations"], c["refinements"], c["num_inliers"])
                assert GF.reprs(pose) == c["model"] and GF.reprs(cam_out) == c["camera"], (model, name)
                assert np.packbits(mask.astype(np.uint8)).tobytes().hex() == c["mask_hex"]
        for name, m1, m2, n, outl, fov in GF.REL_CASES:
            c = G["relative"][name]
            d, x1, x2, c1, c2 = GF.rel_inputs(m1, m2, n, outl, fov, c["data_seed"])
            assert digest([x1, x2]) == c["input_sha256"]
            pose, mask, st = R.estimate_relative_pose(x1, x2, c1, c2, c["options"])
            assert GF.check_rel_run(d, pose, mask), name
            assert (st["iterations"], st["refinements"], st["num_inliers"]) == (c["iterations"], c["refinements"], c["num_inliers"])
            assert GF.reprs(pose) == c["model"], name
            assert np.packbits(mask.astype(np.uint8)).tobytes().hex() == c["mask_hex"]


def test_the_fixture_covers_what_it_says():
    for model in GF.MODELS:
        assert GF.monotone(GF.camera(model), 80.0)
        assert G[model]["unproject"]["disc"]["roundtrip_max_px"] < 1e-6
        wide = G[model]["estimators"]["abs_wide_3000_30"]
        assert wide["fov_deg"] == 150.0 and wide["n"] >= 1024 and wide["num_inliers"] >= 2099  # at most one inlier in 3000 lost
        assert {"abs_focal_1500_30", "abs_refine_1500_50", "abs_1500_30"} <= set(G[model]["estimators"])
    assert len(G["relative"]) == 4


def test_python_surface_knows_the_three_models():
    import poselib_amd as P
    from poselib_amd import synth

    ids = P.api.CAMERA_MODEL_IDS
    assert (ids["OPENCV_FISHEYE"], ids["SIMPLE_RADIAL_FISHEYE"], ids["RADIAL_FISHEYE"]) == (5, 8, 9)
    assert P.Camera("OPENCV_FISHEYE", [900.0, 910.0, 1, 2, 0, 0, 0, 0]).focal() == 905.0
    assert P.Camera("SIMPLE_RADIAL_FISHEYE", [900.0, 1, 2, 0.1]).focal() == 900.0 and P.Camera(9, [800.0, 1, 2, 0.1, 0.2]).model_name() == "RADIAL_FISHEYE"
    pix = np.array([[1500.0, 500.0], [500.0, 500.0], [500.0, -500.0]])  # 45 degrees off the axis, the axis, 45 degrees
    out = synth.fisheye_distort_pixels(pix, "RADIAL_FISHEYE", [1000.0, 500.0, 500.0, -0.1, 0.05])
    th = np.pi / 4
    rd = th * (1 - 0.1 * th ** 2 + 0.05 * th ** 4)
    assert np.allclose(out, [[500.0 + 1000.0 * rd, 500.0], [500.0, 500.0], [500.0, 500.0 - 1000.0 * rd]], rtol=0, atol=1e-9)
    out = synth.fisheye_distort_pixels(pix[:1], "OPENCV_FISHEYE", [1000.0, 1000.0, 500.0, 500.0, 0.0, 0.0, 0.0, 0.0])
    assert np.allclose(out, [[500.0 + 1000.0 * th, 500.0]], rtol=0, atol=1e-9)
    assert "pl_debug_device_math2" in P._lib.EXPORTED_SYMBOLS
