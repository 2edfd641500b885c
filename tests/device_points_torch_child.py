"""Run by tests/test_gpu_device_points.py in a process of its own: torch is imported BEFORE the product library, so both use one
HIP runtime - the order of a program whose matches are torch tensors.  GPU tensors (float32 / float64, contiguous, column and row
views) through the front-ends and a resident problem give the host call's bits; the binding's rejections raise ValueError."""
import os
import sys

import torch  # first: see above

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import poselib_amd as P  # noqa: E402
from poselib_amd import synth  # noqa: E402

KEYS = ("refinements", "iterations", "num_inliers", "inlier_ratio", "model_score", "hypotheses", "inliers")


def blob(m):
    if hasattr(m, "pose"):
        return np.r_[m.pose.q, m.pose.t, m.camera.params].tobytes()
    if hasattr(m, "q"):
        return np.r_[m.q, m.t].tobytes()
    return np.ascontiguousarray(m).tobytes()


def same(got, want, what):
    for k in KEYS:
        assert got[1][k] == want[1][k], (what, k)
    assert blob(got[0]) == blob(want[0]), what


def column_view(x, dtype):
    buf = torch.full((x.shape[0], 5), float("nan"), dtype=dtype, device="cuda")
    buf[:, 1:1 + x.shape[1]] = torch.from_numpy(x).to("cuda").to(dtype)
    return buf[:, 1:1 + x.shape[1]]


def main():
    assert torch.cuda.is_available()
    n = 1300
    h = synth.homography_scene(n, 0.3, 15)
    a, b = h["x1"], h["x2"]
    a32, b32 = a.astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64)
    opt = {"ransac": {"seed": 8}}
    want, want32 = P.estimate_homography(a, b, opt), P.estimate_homography(a32, b32, opt)
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    same(P.estimate_homography(ta, tb, opt), want, "fp64 contiguous")
    same(P.estimate_homography(ta.float(), tb.float(), opt), want32, "fp32 contiguous")
    va = column_view(a, torch.float32)
    assert va.stride(0) == 5 and va.storage_offset() == 1 and va.data_ptr() % 8 == 4
    same(P.estimate_homography(va, column_view(b, torch.float32), opt), want32, "fp32 columns of (N, 5)")
    rows = torch.full((2 * n, 2), float("nan"), dtype=torch.float64, device="cuda")
    rows[::2] = ta
    same(P.estimate_homography(rows[::2], column_view(b, torch.float64), opt), want, "fp64 every second row")
    same(P.estimate_homography(ta.t().contiguous().t(), tb, opt), want, "column stride 2: made contiguous on the device")
    same(P.estimate_homography(torch.from_numpy(a), torch.from_numpy(b), opt), want, "CPU tensors: the host path")

    d = synth.absolute_pose_scene(n, 0.3, 11)
    want = P.estimate_absolute_pose(d["p2d"], d["p3d"], d["camera"], {"ransac": {"seed": 3}})
    same(P.estimate_absolute_pose(column_view(d["p2d"], torch.float64), column_view(d["p3d"], torch.float64), d["camera"],
                                  {"ransac": {"seed": 3}}), want, "absolute pose, views")

    host = P.Problem(P.KIND_HOM, a, b)
    dev32 = P.Problem(P.KIND_HOM, va, tb.float())
    same(dev32.run(opt), P.Problem(P.KIND_HOM, a32, b32).run(opt), "resident problem, fp32")
    dev64 = P.Problem(P.KIND_HOM, ta, column_view(b, torch.float64))
    same(dev64.run(opt), host.run(opt), "resident problem, fp64")
    got = P.ransac_batch([dev64, host], [opt, opt])
    same(got[0], host.run(opt), "batch, device-created")
    same(got[1], host.run(opt), "batch, host-created")

    for bad in (torch.float16, torch.int32, torch.int64):
        try:
            P.estimate_homography(ta.to(bad), tb.to(bad))
            raise SystemExit(f"{bad} accepted")
        except ValueError:
            pass
    for x, y in ((ta, b), (a, tb)):
        try:
            P.estimate_homography(x, y)
            raise SystemExit("host and device points mixed")
        except ValueError:
            pass
    if torch.cuda.device_count() > 1:
        try:
            P.estimate_homography(ta.to("cuda:1"), tb.to("cuda:1"))
            raise SystemExit("tensors of another device accepted")
        except ValueError:
            pass
    print("torch child ok")


if __name__ == "__main__":
    main()
