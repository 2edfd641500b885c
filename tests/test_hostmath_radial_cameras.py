"""SIMPLE_RADIAL and RADIAL cameras on the CPU: the device math headers (pl_refine.h, pl_refine_cam.h) compiled for the host
(tests/hostmath) against the reference's own camera models and bundle adjustment, bit for bit.

The comparator is tests/golden/golden_cameras_v1.json, recorded from the reference build (oracle/_ref) by
tests/golden/make_golden_cameras.py; where that build is present the fixture is also held to it, entry for entry.  The oracle's
restatement (liboracle.so) does not know these models and is never called with them here.

A library without the two models sends them through the NULL-camera branch of every switch: these tests then fail.
"""
import json

import numpy as np
import pytest

import hostmath_lib as HM
import ref_lib
from golden import make_golden_cameras as GC
from golden.make_golden import digest

G = json.load(open(GC.PATH))
LOSS_IDS = {"TRIVIAL": 0, "TRUNCATED": 1, "HUBER": 2, "CAUCHY": 3}


def hm_camera(cam):
    return HM.camera_params(cam["model"], cam["params"])


def flag_bits(bo):
    return (1 if bo.get("refine_focal_length") else 0) | (2 if bo.get("refine_principal_point") else 0) | (4 if bo.get("refine_extra_params") else 0)


def hm_options(bo):
    return HM.lm_options(bo.get("max_iterations", 100), LOSS_IDS[bo["loss_type"]], bo["loss_scale"])


@pytest.mark.parametrize("model", sorted(GC.MODELS))
@pytest.mark.parametrize("name", ["disc", "centre", "k0"])
def test_unproject_equals_the_reference_bit_for_bit(model, name):
    """10 000 pixels at a radius of up to 1.0, the principal point, points within 1e-9 of it and on either side of r0 = 1e-8, k = 0"""
    cam, pix = GC.unproject_inputs(model)[name]
    want = G[model]["unproject"][name]
    assert digest([pix]) == want["input_sha256"], "the inputs changed: regenerate the fixture"
    assert len(pix) == {"disc": 10000, "centre": 41, "k0": 2000}[name]
    got = HM.unproject(hm_camera(cam), pix)
    assert GC.reprs(got[:48]) == want["head"]
    assert digest([got]) == want["sha256"]
    assert digest([GC.undistorted_pixels(cam, got)]) == want["undistorted_sha256"]
    if name == "centre":
        assert got[0].tolist() == [0.0, 0.0]
        r0 = np.hypot(*((pix - [GC.CX, GC.CY]) / GC.F).T)
        assert (r0 <= 1e-8).sum() >= 15 and (r0 > 1e-8).sum() >= 15  # both sides of the reference's test
    if name == "disc":  # ... and it is the inverse of the distortion
        assert np.abs(synth_back(cam, got) - pix).max() < 1e-6
        assert np.abs(got - (pix - [GC.CX, GC.CY]) / GC.F).max() > 0.02  # (far from the linear camera's answer)


def synth_back(cam, un):
    from poselib_amd import synth

    return synth.radial_distort_pixels(GC.undistorted_pixels(cam, un), cam["params"])


@pytest.mark.parametrize("model", sorted(GC.MODELS))
@pytest.mark.parametrize("n", GC.SMALL_N + GC.LARGE_N)
def test_bundle_adjustment_equals_the_reference_bit_for_bit(model, n):
    """hm_lm with a camera (the pose alone) and hm_lm_cam (intrinsics with the pose): pose, camera parameters and iteration count.
    Up to 256 correspondences: the five flag sets, CAUCHY and HUBER; beyond: with and without a mask.  The serial host statement
    sums in the reference's order at every n, so the larger problems are bit for bit here as well."""
    pix, X, gt, cam0, p0 = GC.bundle_inputs(model, n)
    rec = G[model]["bundle"]
    assert digest([pix, X, p0, cam0["params"]]) == rec[f"{n}/input_sha256"], "the inputs changed: regenerate the fixture"
    cols = [pix[:, 0], pix[:, 1], X[:, 0], X[:, 1], X[:, 2]]
    runs = GC.bundle_runs(n)
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
            assert GC.reprs(cam) != GC.reprs(cam0["params"])  # the camera did move
        assert it == want["iterations"], (model, n, key, it, want["iterations"])
        assert GC.reprs(got[:7]) == want["pose"], (model, n, key)
        assert GC.reprs(cam) == want["camera"], (model, n, key)
        assert it >= 2


def test_refinement_indices_follow_the_reference_order():
    """get_param_refinement_idx: focal {0}, principal point {1, 2}, extra {3} / {3, 4} - seen through which parameters a run moves"""
    for model, extra in (("SIMPLE_RADIAL", [3]), ("RADIAL", [3, 4])):
        pix, X, gt, cam0, p0 = GC.bundle_inputs(model, 64)
        cols = [pix[:, 0], pix[:, 1], X[:, 0], X[:, 1], X[:, 2]]
        for flags, moved in ((1, [0]), (2, [1, 2]), (4, extra), (7, [0, 1, 2] + extra)):
            _, cam, _, _ = HM.lm_cam(cols, p0, HM.lm_options(20, 3, 1.0), hm_camera(cam0), flags)
            assert [i for i in range(len(cam)) if cam[i] != cam0["params"][i]] == moved, (model, flags)


@pytest.mark.skipif(not ref_lib.available(), reason="oracle/_ref not built and the reference sources absent")
@pytest.mark.parametrize("part", ["unproject", "bundle"])
def test_fixture_equals_the_live_reference(part):
    live = GC.record(parts=(part,))
    for model in GC.MODELS:
        assert live[model][part] == G[model][part], (model, part)


@pytest.mark.skipif(not ref_lib.available(), reason="oracle/_ref not built and the reference sources absent")
def test_fixture_estimator_runs_equal_the_live_reference_and_are_successful_matches():
    """every recorded RANSAC run again, with its recorded seeds: same decisions, same model bit for bit - and a match that found the
    ground truth (the generator's own condition)"""
    with ref_lib.reference() as R:
        for model in GC.MODELS:
            for name, n, outl, opt, start in GC.ABS_CASES:
                c = G[model]["estimators"][name]
                d, pix, cam_in = GC.abs_inputs(model, n, outl, start, c["data_seed"])
                assert digest([pix, d["p3d"]]) == c["input_sha256"]
                pose, mask, st, cam_out = R.estimate_absolute_pose(pix, d["p3d"], cam_in, c["options"], return_camera=True)
                assert GC.check_abs_run(d, pose, mask, cam_out), (model, name)
                assert (st["iterations"], st["refinements"], st["num_inliers"]) == (c["iterations"], c["refinements"], c["num_inliers"])
                assert GC.reprs(pose) == c["model"] and GC.reprs(cam_out) == c["camera"], (model, name)
                assert np.packbits(mask.astype(np.uint8)).tobytes().hex() == c["mask_hex"]
        for name, m1, m2, n, outl in GC.REL_CASES:
            c = G["relative"][name]
            d, x1, x2, c1, c2 = GC.rel_inputs(m1, m2, n, outl, c["data_seed"])
            assert digest([x1, x2]) == c["input_sha256"]
            pose, mask, st = R.estimate_relative_pose(x1, x2, c1, c2, c["options"])
            assert GC.check_rel_run(d, pose, mask), name
            assert (st["iterations"], st["refinements"], st["num_inliers"]) == (c["iterations"], c["refinements"], c["num_inliers"])
            assert GC.reprs(pose) == c["model"], name
            assert np.packbits(mask.astype(np.uint8)).tobytes().hex() == c["mask_hex"]


def test_python_surface_knows_the_two_models():
    import poselib_amd as P
    from poselib_amd import synth

    assert P.api.CAMERA_MODEL_IDS["SIMPLE_RADIAL"] == 2 and P.api.CAMERA_MODEL_IDS["RADIAL"] == 3
    assert P.Camera("SIMPLE_RADIAL", [900.0, 1, 2, 0.1]).focal() == 900.0 and P.Camera("RADIAL", [800.0, 1, 2, 0.1, 0.2]).focal() == 800.0
    assert P.Camera(3, [800.0, 1, 2, 0.1, 0.2]).model_name() == "RADIAL"
    pix = np.array([[700.0, 400.0], [500.0, 500.0]])
    out = synth.radial_distort_pixels(pix, [1000.0, 500.0, 500.0, -0.1, 0.05])
    r2 = 0.2 ** 2 + 0.1 ** 2
    assert np.allclose(out[0], 500.0 + np.array([200.0, -100.0]) * (1 - 0.1 * r2 + 0.05 * r2 * r2)) and out[1].tolist() == [500.0, 500.0]
