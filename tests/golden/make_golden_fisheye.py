#!/usr/bin/env python
"""Generates tests/golden/golden_fisheye_v1.json - frozen outputs of the reference for the fisheye camera models
OPENCV_FISHEYE (id 5), SIMPLE_RADIAL_FISHEYE (id 8) and RADIAL_FISHEYE (id 9): un-projection, bundle adjustment with and without
refined intrinsics, estimate_absolute_pose and estimate_relative_pose.

PROVENANCE: produced by the REFERENCE'S OWN SOURCES - oracle/_ref, the reference compiled in place against oracle/eigen_shim
(oracle/Makefile.ref), driven through tests/ref_lib.py - on the CPU, and frozen, exactly as make_golden_cameras.py does for the
radial models (whose helpers are reused).  The oracle's restatement (liboracle.so) does not know these models and is never called
with them.  Inputs are regenerated from poselib_amd.synth seeds and numpy's RandomState; large outputs are stored as SHA-256
digests of their bytes, small ones as repr() of every double.
tests/test_hostmath_fisheye_cameras.py holds the device headers (host build) to the fixture bit for bit and the fixture to the live
reference where it can be built; tests/test_gpu_fisheye_cameras.py holds the HIP path to it.

Conditions main() asserts, so that the fixture never encodes a failure: the un-projection of the disc inverts
synth.fisheye_distort_pixels to 1e-6 px; every RANSAC case recovers the ground truth (check_abs_run / check_rel_run of the radial
generator), else the next seed is tried; the distortion coefficients give a monotone theta -> rd over the field of view.
Re-run (needs the reference build):
    python tests/golden/make_golden_fisheye.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import ref_lib  # noqa: E402
from golden import make_golden_cameras as GC  # noqa: E402
from golden.make_golden_cameras import FLAGS, LARGE_N, SMALL_N, bundle_runs, check_abs_run, check_rel_run, reprs, start_pose  # noqa: E402,F401
from golden.make_golden import digest  # noqa: E402
from poselib_amd import synth  # noqa: E402

PATH = os.path.join(HERE, "golden_fisheye_v1.json")
MODELS = {"OPENCV_FISHEYE": 5, "SIMPLE_RADIAL_FISHEYE": 8, "RADIAL_FISHEYE": 9}
NAMES = {v: k for k, v in MODELS.items()}
F, CX, CY = GC.F, GC.CX, GC.CY
PARAMS = {"OPENCV_FISHEYE": [1000.0, 1010.0, 500.0, 500.0, -0.02, 0.005, -0.001, 0.0002],
          "SIMPLE_RADIAL_FISHEYE": [1000.0, 500.0, 500.0, -0.03],
          "RADIAL_FISHEYE": [1000.0, 500.0, 500.0, -0.03, 0.004]}
N_FOCAL = {"OPENCV_FISHEYE": 2, "SIMPLE_RADIAL_FISHEYE": 1, "RADIAL_FISHEYE": 1}  # parameters before the principal point
HALF_ANGLE_DEG = 75.0  # the un-projection's disc; the widest scene (150 degrees field of view) reaches 79 degrees in its corners
WIDE_FOV_DEG = 150.0


def camera(model, extra=None):
    """the camera as a dict with the INTEGER model id (tests/oracle_lib.py has no names for these models)"""
    par = list(PARAMS[model])
    k0 = N_FOCAL[model] + 2
    if extra is not None:
        par[k0:] = list(extra)
    return {"model": MODELS[model], "width": int(2 * CX), "height": int(2 * CY), "params": par}


def named(cam):
    """the same camera for poselib_amd, which knows the names"""
    return dict(cam, model=NAMES[cam["model"]])


def layout(cam):
    """fx, fy, cx, cy, [k ...] of a camera dict"""
    p, nf = cam["params"], N_FOCAL[NAMES[cam["model"]]]
    return p[0], p[nf - 1], p[nf], p[nf + 1], list(p[nf + 2:])


def monotone(cam, max_deg):
    """theta -> rd = theta (1 + k1 theta^2 + ...) grows all the way to max_deg"""
    ks = layout(cam)[4]
    th = np.linspace(0.0, np.radians(max_deg), 2000)
    d = np.ones_like(th)
    for j, k in enumerate(ks):
        d += (2 * j + 3) * k * th ** (2 * j + 2)
    return bool((d > 0.05).all())


def through(cam, pinhole_pix):
    """pixels of the synthetic scenes' SIMPLE_PINHOLE camera (F, CX, CY) as the fisheye camera sees the same rays"""
    fx, fy, cx, cy, _ = layout(cam)
    pix = np.stack([(pinhole_pix[:, 0] - CX) / F * fx + cx, (pinhole_pix[:, 1] - CY) / F * fy + cy], axis=1)
    return synth.fisheye_distort_pixels(pix, NAMES[cam["model"]], cam["params"])


def undistorted_pixels(cam, un):
    """pl_undistort_points' output for the un-projected points `un`: the pixel of the distortion-free camera (one multiplication
    and one addition per coordinate, IEEE)"""
    fx, fy, cx, cy, _ = layout(cam)
    return np.stack([fx * un[:, 0] + cx, fy * un[:, 1] + cy], axis=1)


# ------------------------------------------------------------------------------------------ un-projection
def unproject_inputs(model):
    """name -> (camera, pixels).  `disc`: 10 000 pixels of rays up to 75 degrees from the axis; `centre`: the principal point itself
    and rings at 1e-9 .. 1e-7 on either side of the reference's rd > 1e-8 test; `k0`: all-zero distortion"""
    cam = camera(model)
    fx, fy, cx, cy, ks = layout(cam)
    rs = np.random.RandomState(40 + MODELS[model])
    theta = np.radians(HALF_ANGLE_DEG) * np.sqrt(rs.rand(10000))
    a = 2.0 * np.pi * rs.rand(10000)
    rd = theta.copy()
    for j, k in enumerate(ks):
        rd += k * theta ** (2 * j + 3)
    disc = np.stack([fx * rd * np.cos(a) + cx, fy * rd * np.sin(a) + cy], axis=1)
    offs = [(0.0, 0.0)]
    for rad in (1e-9, 5e-10, 9e-9, 0.99e-8, 1.0e-8, 1.01e-8, 2e-8, 1e-7):
        for ang in (0.0, 0.7, 2.1, 3.9, 5.5):
            offs.append((rad * np.cos(ang), rad * np.sin(ang)))
    centre = np.array([[fx * u + cx, fy * v + cy] for u, v in offs])
    flat = np.stack([fx * theta[:2000] * np.cos(a[:2000]) + cx, fy * theta[:2000] * np.sin(a[:2000]) + cy], axis=1)
    return {"disc": (cam, disc), "centre": (cam, centre), "k0": (camera(model, [0.0] * len(ks)), flat)}


def record_unproject(R, model):
    out = {}
    for name, (cam, pix) in unproject_inputs(model).items():
        un = R.unproject(cam, pix)
        rec = {"input_sha256": digest([pix]), "sha256": digest([un]), "undistorted_sha256": digest([undistorted_pixels(cam, un)]),
               "head": reprs(un[:48])}
        if name == "disc":  # the issue's check: un-projection inverts the distortion
            back = synth.fisheye_distort_pixels(undistorted_pixels(cam, un), model, cam["params"])
            rec["roundtrip_max_px"] = float(np.abs(back - pix).max())
            assert rec["roundtrip_max_px"] < 1e-6, rec
        out[name] = rec
    return out


# ------------------------------------------------------------------------------------------ bundle adjustment
def off_calibration(cam, rs, rel, pp):
    par = np.array(cam["params"], dtype=np.float64)
    nf = N_FOCAL[NAMES[cam["model"]]]
    par[:nf] *= 1.0 + rel * rs.randn()
    par[nf:nf + 2] += pp * rs.randn(2)
    return dict(cam, params=[float(v) for v in par])


def bundle_inputs(model, n):
    """the scene of the radial fixture's bundle tests seen through the fisheye camera: (pixels, 3-D points, mask of the ground-truth
    inliers, camera off its calibration, starting pose)"""
    small = n <= 256
    rs = np.random.RandomState((300 if small else 400) + n + MODELS[model])
    d = synth.absolute_pose_scene(n, 0.0 if small else 0.3, (5200 if small else 5300) + n)
    cam = camera(model)
    pix = through(cam, np.asarray(d["p2d"]))
    p0 = start_pose(d, rs, 0.003 if small else 0.002)
    return pix, np.asarray(d["p3d"]), d["inlier_gt"], off_calibration(cam, rs, 0.02, 3.0), p0


def record_bundle(R, model):
    out = {}
    for n in SMALL_N + LARGE_N:
        pix, X, gt, cam0, p0 = bundle_inputs(model, n)
        for key, bo, masked in bundle_runs(n):
            sel = gt if masked else slice(None)
            if key.startswith("pose"):
                pose, st = R.bundle_adjust(pix[sel], X[sel], cam0, p0, bo)
                cam = cam0["params"]
            else:
                pose, cam, st = R.bundle_adjust_camera(pix[sel], X[sel], cam0, p0, bo)
            out[f"{n}/{key}"] = {"iterations": int(st.iterations), "pose": reprs(pose), "camera": reprs(cam),
                                 "initial_cost": repr(float(st.initial_cost)), "cost": repr(float(st.cost))}
        out[f"{n}/input_sha256"] = digest([pix, X, p0, cam0["params"]])
    return out


# ------------------------------------------------------------------------------------------ estimators
#           name, n, outlier ratio, field of view, options, camera the call starts from: (relative focal error, principal point shift)
ABS_CASES = [
    ("abs_1500_30", 1500, 0.3, 80.0, {"max_error": 2.0}, None),
    ("abs_400_50", 400, 0.5, 80.0, {"max_error": 2.0}, None),
    ("abs_wide_3000_30", 3000, 0.3, WIDE_FOV_DEG, {"max_error": 2.0}, None),
    ("abs_wide_200_50", 200, 0.5, WIDE_FOV_DEG, {"max_error": 2.0}, None),
    # (a fisheye image un-projected with a wrong focal length is no pinhole image of another focal length: ransac_pnpf sees a
    # residual distortion that grows with the error of the starting focal length and with the field of view - 1 % at 70 degrees
    # leaves about 2 px at the corners, inside the threshold; the radial fixture's 5 % would cost the corners their inliers)
    ("abs_focal_1500_30", 1500, 0.3, 70.0, {"max_error": 6.0, "estimate_focal_length": True}, (0.01, 0.0)),
    ("abs_focal_400_30", 400, 0.3, 70.0, {"max_error": 6.0, "estimate_focal_length": True}, (-0.01, 0.0)),
    ("abs_refine_1500_50", 1500, 0.5, 80.0, {"max_error": 8.0, "bundle": dict(FLAGS[4])}, (0.002, 1.0)),
    ("abs_refine_400_30", 400, 0.3, 80.0, {"max_error": 8.0, "bundle": dict(FLAGS[2])}, (-0.002, 1.0)),
]
#           name, model of camera 1, model of camera 2 (None: SIMPLE_PINHOLE), n, outlier ratio, field of view
REL_CASES = [
    ("rel_fisheye_pinhole_1500_30", "OPENCV_FISHEYE", None, 1500, 0.3, 70.0),
    ("rel_fisheye_pinhole_400_50", "RADIAL_FISHEYE", None, 400, 0.5, 70.0),
    ("rel_two_fisheye_1500_50", "RADIAL_FISHEYE", "SIMPLE_RADIAL_FISHEYE", 1500, 0.5, 80.0),
    ("rel_two_fisheye_wide_1200_30", "OPENCV_FISHEYE", "SIMPLE_RADIAL_FISHEYE", 1200, 0.3, 120.0),
]
REL_MAX_ERROR = GC.REL_MAX_ERROR


def abs_inputs(model, n, outl, fov, start, data_seed):
    d = synth.absolute_pose_scene(n, outl, data_seed, fov_deg=fov)
    cam = camera(model)
    pix = through(cam, np.asarray(d["p2d"]))
    cam_in = cam
    if start is not None:
        rel, pp = start
        par, nf = list(cam["params"]), N_FOCAL[model]
        for i in range(nf):
            par[i] *= 1.0 + rel
        par[nf] += pp
        par[nf + 1] -= pp
        cam_in = dict(cam, params=par)
    return d, pix, cam_in


def rel_inputs(m1, m2, n, outl, fov, data_seed):
    d = synth.relative_pose_scene(n, outl, data_seed, fov_deg=fov)
    c1 = camera(m1)
    x1 = through(c1, np.asarray(d["x1"]))
    if m2 is None:
        return d, x1, np.asarray(d["x2"]), c1, d["camera2"]
    c2 = camera(m2)
    return d, x1, through(c2, np.asarray(d["x2"])), c1, c2


def record_estimators(R, model):
    out = {}
    base = 8000 + 100 * MODELS[model]
    for k, (name, n, outl, fov, opt, start) in enumerate(ABS_CASES):
        for attempt in range(40):
            data_seed, seed = base + k + 1000 * (attempt // 4), 1 + attempt % 4
            d, pix, cam_in = abs_inputs(model, n, outl, fov, start, data_seed)
            o = dict(opt, ransac={"seed": seed})
            pose, mask, st, cam_out = R.estimate_absolute_pose(pix, d["p3d"], cam_in, o, return_camera=True)
            if check_abs_run(d, pose, mask, cam_out):
                break
        else:
            raise AssertionError(f"{model} {name}: the reference did not recover the ground truth for any seed tried")
        assert check_abs_run(d, pose, mask, cam_out)
        out[name] = {"n": n, "outlier_ratio": outl, "fov_deg": fov, "data_seed": data_seed, "options": o, "start": start,
                     "input_sha256": digest([pix, d["p3d"]]), "iterations": st["iterations"], "refinements": st["refinements"],
                     "num_inliers": st["num_inliers"], "model_score": repr(float(st["model_score"])), "model": reprs(pose),
                     "camera": reprs(cam_out), "mask_hex": np.packbits(mask.astype(np.uint8)).tobytes().hex()}
        print(model, name, data_seed, seed, st["iterations"], st["refinements"], st["num_inliers"], int(d["inlier_gt"].sum()))
    return out


def record_relative(R):
    out = {}
    for k, (name, m1, m2, n, outl, fov) in enumerate(REL_CASES):
        for attempt in range(40):
            data_seed, seed = 8500 + k + 1000 * (attempt // 4), 1 + attempt % 4
            d, x1, x2, c1, c2 = rel_inputs(m1, m2, n, outl, fov, data_seed)
            o = {"max_error": REL_MAX_ERROR, "ransac": {"seed": seed}}
            pose, mask, st = R.estimate_relative_pose(x1, x2, c1, c2, o)
            if check_rel_run(d, pose, mask):
                break
        else:
            raise AssertionError(f"{name}: the reference did not recover the ground truth for any seed tried")
        assert check_rel_run(d, pose, mask)
        out[name] = {"n": n, "outlier_ratio": outl, "fov_deg": fov, "data_seed": data_seed, "options": o, "models": [m1, m2],
                     "input_sha256": digest([x1, x2]), "iterations": st["iterations"], "refinements": st["refinements"],
                     "num_inliers": st["num_inliers"], "model_score": repr(float(st["model_score"])), "model": reprs(pose),
                     "mask_hex": np.packbits(mask.astype(np.uint8)).tobytes().hex()}
        print(name, data_seed, seed, st["iterations"], st["refinements"], st["num_inliers"], int(d["inlier_gt"].sum()))
    return out


def record(parts=("unproject", "bundle", "estimators", "relative")):
    """the fixture (or the named parts of it) from the live reference build"""
    assert ref_lib.available(), "the fixtures are generated through oracle/_ref: needs the reference build"
    out = {"provenance": "generated by the reference's own sources (oracle/_ref against oracle/eigen_shim); see make_golden_fisheye.py"}
    with ref_lib.reference() as R:
        for model in MODELS:
            assert monotone(camera(model), 80.0), model
            out[model] = {}
            if "unproject" in parts:
                out[model]["unproject"] = record_unproject(R, model)
            if "bundle" in parts:
                out[model]["bundle"] = record_bundle(R, model)
            if "estimators" in parts:
                out[model]["estimators"] = record_estimators(R, model)
        if "relative" in parts:
            out["relative"] = record_relative(R)
    return out


def main():
    with open(PATH, "w") as f:
        json.dump(record(), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
