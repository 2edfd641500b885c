"""BASELINE config 3 "OPENCV camera model": the homography / 7-point estimators take no camera (robust.h:112-113,
133-134), so pixels of a distorting camera are un-distorted first - Camera::unproject per point
(misc/camera_models.cc:1025-1032, iterative inverse :972-990) - as a stage of its own on the device
(pl_undistort_points), then fed to estimate_homography / estimate_fundamental.  Checked against the oracle's unproject
and the oracle's estimators on the same un-distorted points."""
import numpy as np
import pytest

import oracle_lib as O
from poselib_amd import synth

pytestmark = pytest.mark.gpu

OPENCV = {"model": "OPENCV", "width": 1000, "height": 1000,
          "params": [1000.0, 1010.0, 500.0, 505.0, 0.04, -0.015, 8e-4, -6e-4]}


def _pinhole_pixels(cam, un):
    fx, fy, cx, cy = cam["params"][:4]
    return np.c_[fx * un[:, 0] + cx, fy * un[:, 1] + cy]


@pytest.mark.parametrize("kind", ["hom", "fund"])
def test_undistort_stage_in_front_of_the_two_view_estimators(gpu, kind):
    d = (synth.homography_scene if kind == "hom" else synth.fundamental_scene)(10000, 0.5, 1003 if kind == "hom" else 1004)
    # the scene's pinhole pixels seen through the distorting camera
    pin = {"model": "PINHOLE", "params": [1000.0, 1000.0, 500.0, 500.0]}
    x1d = synth.opencv_distort_pixels(_pinhole_pixels(OPENCV, O.unproject(pin, d["x1"])), OPENCV["params"])
    x2d = synth.opencv_distort_pixels(_pinhole_pixels(OPENCV, O.unproject(pin, d["x2"])), OPENCV["params"])
    u1, u2 = gpu.undistort_points(OPENCV, x1d), gpu.undistort_points(OPENCV, x2d)
    r1, r2 = _pinhole_pixels(OPENCV, O.unproject(OPENCV, x1d)), _pinhole_pixels(OPENCV, O.unproject(OPENCV, x2d))
    err = max(np.abs(u1 - r1).max(), np.abs(u2 - r2).max())
    print(kind, "max |device - oracle| of the un-distorted pixels:", err)
    assert err == 0.0  # the same IEEE operations in the same order (no libm call besides sqrt)
    # the distortion was real and the stage removes it
    assert np.abs(x1d - _pinhole_pixels(OPENCV, O.unproject(pin, d["x1"]))).max() > 1.0
    assert np.abs(u1 - _pinhole_pixels(OPENCV, O.unproject(pin, d["x1"]))).max() < 1e-6
    opt = {"ransac": {"seed": 2}}
    if kind == "hom":
        M, info = gpu.estimate_homography(u1, u2, opt)
        Mo, mask, st = O.estimate_homography(r1, r2, opt)
    else:
        M, info = gpu.estimate_fundamental(u1, u2, opt)
        Mo, mask, st = O.estimate_fundamental(r1, r2, opt)
    assert info["iterations"] == st["iterations"] and info["refinements"] == st["refinements"]
    assert info["num_inliers"] == st["num_inliers"] and (np.array(info["inliers"]) == mask).all()
    assert info["num_inliers"] > 2500
    A, B = M / np.linalg.norm(M), Mo / np.linalg.norm(Mo)
    assert np.linalg.norm(A - B) < 1e-6  # sign included


def test_undistort_rejects_what_it_does_not_cover(gpu):
    import poselib_amd as P

    with pytest.raises(P.PoseLibAmdError):
        P.undistort_points({"model": "NULL", "params": []}, np.zeros((4, 2)))
    assert P.undistort_points(OPENCV, np.zeros((0, 2))).shape == (0, 2)
    p = np.array([[500.0, 505.0], [10.0, 990.0]])
    sp = {"model": "SIMPLE_PINHOLE", "params": [800.0, 400.0, 300.0]}
    assert np.abs(P.undistort_points(sp, p) - p).max() < 1e-12  # a linear camera maps onto itself


UNDISTORT_CAMERAS = [
    {"model": "OPENCV", "width": 1280, "height": 720, "params": [800.0, 820.0, 640.0, 360.0, -0.3, 0.01, 1e-3, -2e-3]},
    {"model": "OPENCV", "width": 1280, "height": 720, "params": [800.0, 780.0, 640.0, 360.0, 0.3, -0.05, -1.5e-3, 1e-3]},
    {"model": "PINHOLE", "width": 1280, "height": 720, "params": [900.0, 600.0, 640.5, 360.25]},
]


def _hostile_pixels(cam):
    """the principal point, the image's corners at 1x and 3x its size, 1e6 px, NaN / inf, and a grid out to 3.5x the
    image size - beyond the fold of a strong distortion, where the Newton inverse runs all 100 iterations or diverges"""
    w, h = cam["width"], cam["height"]
    cx, cy = cam["params"][2:4]
    pts = [(cx, cy)]
    for s in (1.0, 3.0):
        for a in (-0.5, 0.5):
            for b in (-0.5, 0.5):
                pts.append((cx + s * a * w, cy + s * b * h))
    for a in (-1e6, 0.0, 1e6):
        for b in (-1e6, 0.0, 1e6):
            pts.append((cx + a, cy + b))
    for bad in (np.nan, np.inf, -np.inf):
        pts += [(bad, cy), (cx, bad), (bad, bad), (bad, 1e6)]
    gx, gy = np.meshgrid(np.linspace(cx - 3.5 * w, cx + 3.5 * w, 301), np.linspace(cy - 3.5 * h, cy + 3.5 * h, 301))
    return np.r_[np.array(pts, dtype=np.float64), np.c_[gx.ravel(), gy.ravel()]]


def _same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


@pytest.mark.parametrize("ci", range(len(UNDISTORT_CAMERAS)))
def test_undistort_hostile_pixels_bit_for_bit(gpu, ci):
    """pl_undistort_points against the oracle's Camera::unproject and the host compile of camera_unproject (pl_refine.h)
    on pixels far outside the image, where the iterative inverse does not converge, and on NaN / inf: every bit equal, a
    NaN equal to a NaN"""
    import hostmath_lib as HM

    cam = UNDISTORT_CAMERAS[ci]
    pix = _hostile_pixels(cam)
    got = gpu.undistort_points(cam, pix)
    fx, fy, cx, cy = cam["params"][:4]
    with np.errstate(invalid="ignore", over="ignore"):
        ref = _pinhole_pixels(cam, O.unproject(cam, pix))
        mid = {"PINHOLE": 1, "OPENCV": 4}[cam["model"]]
        hm = HM.unproject(HM.camera_params(mid, cam["params"]), pix)
        hm = np.c_[fx * hm[:, 0] + cx, fy * hm[:, 1] + cy]
    for name, want in (("oracle", ref), ("host compile", hm)):
        same = _same_bits(got, want).all(axis=1)
        i = int(np.argmin(same))
        assert same.all(), (name, int((~same).sum()), pix[i].tolist(), got[i].tolist(), want[i].tolist())
    assert np.isnan(got[~np.isfinite(pix).all(axis=1)]).any()
    if cam["model"] == "OPENCV":
        # the set holds pixels whose inverse did not converge: pushed through the distortion again they miss the input
        with np.errstate(invalid="ignore", over="ignore"):
            back = synth.opencv_distort_pixels(got, cam["params"])
            miss = ~(np.abs(back - pix) < 1e-6).all(axis=1) & np.isfinite(pix).all(axis=1)
        print(cam["params"][4:], "pixels without a converged inverse:", int(miss.sum()), "of", pix.shape[0])
        assert miss.sum() > 1000
