"""Run by tests/test_gpu_device_masks.py in a process of its own: torch is imported BEFORE the product library, so both use one HIP
runtime.  The config-3 pipeline on tensors, nothing of which passes through the host: ONE padded (pairs, N, 5) float32 CUDA tensor
of distorted matches and confidences -> undistort_points (a new float64 tensor, and out= views) -> estimate_batch with
"inliers_out": mask[i], a row of a (pairs, N) torch.bool tensor -> m[i][mask[i]] on the device.  Everything equals the numpy path."""
import os
import sys

import torch  # first: see above

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import poselib_amd as P  # noqa: E402
from poselib_amd import synth  # noqa: E402

KEYS = ("n_used", "refinements", "iterations", "num_inliers", "inlier_ratio", "model_score", "hypotheses")
PAIRS, N = 4, 256
OPENCV = {"model": "OPENCV", "width": 1000, "height": 1000, "params": [1000.0, 1010.0, 500.0, 505.0, 0.04, -0.015, 8e-4, -6e-4]}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def main():
    if not torch.cuda.is_available():
        print("torch sees no GPU")
        return
    host = np.zeros((PAIRS, N, 5), dtype=np.float32)
    rng = np.random.default_rng(4)
    for i in range(PAIRS):
        h = synth.homography_scene(N, 0.3, 80 + i)
        host[i, :, :2] = synth.opencv_distort_pixels(h["x1"], OPENCV["params"])
        host[i, :, 2:4] = synth.opencv_distort_pixels(h["x2"], OPENCV["params"])
        host[i, :, 4] = np.round((h["inlier_gt"] + 0.4 * rng.standard_normal(N)) * 16) / 16
        host[i, N - 20 * i:, 4] = np.nan  # padding rows, another number per pair
    wide = host.astype(np.float64)
    m = torch.from_numpy(host).cuda()
    opts = [{"ransac": {"max_iterations": 2000, "min_iterations": 100, "seed": 7 + i}} for i in range(PAIRS)]

    # ---- the numpy path: host undistortion, host scores, masks as lists
    u1 = [P.undistort_points(OPENCV, wide[i, :, :2]) for i in range(PAIRS)]
    u2 = [P.undistort_points(OPENCV, wide[i, :, 2:4]) for i in range(PAIRS)]
    want = P.estimate_batch([("hom", u1[i], u2[i], dict(opts[i], scores=host[i, :, 4], min_score=0.25)) for i in range(PAIRS)])
    want_report = P.last_batch_report()

    # ---- undistort_points on tensors: a new float64 tensor on the same device; out= views; the grouped form; in place
    t = P.undistort_points(OPENCV, m[0, :, :2])
    assert isinstance(t, torch.Tensor) and t.dtype == torch.float64 and t.device == m.device and tuple(t.shape) == (N, 2)
    assert (bits(t.cpu().numpy()) == bits(u1[0])).all()
    clean = torch.full((PAIRS, N, 4), -7.0, dtype=torch.float64, device="cuda")
    outs = P.undistort_points_batch([(OPENCV, m[i, :, 2 * v:2 * v + 2], clean[i, :, 2 * v:2 * v + 2]) for i in range(PAIRS) for v in (0, 1)])
    assert outs[3] is not None and outs[3].data_ptr() == clean[1, :, 2:4].data_ptr()
    back = clean.cpu().numpy()
    for i in range(PAIRS):
        assert (bits(back[i, :, :2]) == bits(u1[i])).all() and (bits(back[i, :, 2:]) == bits(u2[i])).all(), i
    again = clean[2, :, :2].clone()
    assert P.undistort_points({"model": "PINHOLE", "params": OPENCV["params"][:4]}, again, out=again) is again  # in place, a linear camera
    assert torch.allclose(again, clean[2, :, :2], rtol=0, atol=1e-9)
    fresh = P.undistort_points_batch([(OPENCV, m[1, :, :2], None)])[0]
    assert fresh.dtype == torch.float64 and (bits(fresh.cpu().numpy()) == bits(u1[1])).all()

    # ---- estimate_batch with the masks on the device
    mask = torch.zeros((PAIRS, N), dtype=torch.bool, device="cuda")
    mask[:] = True  # (whatever it held: all N flags of every row are written)
    got = P.estimate_batch([("hom", clean[i, :, :2], clean[i, :, 2:4], dict(opts[i], scores=m[i, :, 4], min_score=0.25, inliers_out=mask[i]))
                            for i in range(PAIRS)])
    assert P.last_batch_report() == want_report and want_report["grouped"] == PAIRS, (P.last_batch_report(), want_report)
    flags = mask.cpu().numpy()
    for i, (g, w) in enumerate(zip(got, want)):
        assert w[1]["num_inliers"] > 0.3 * w[1]["n_used"], i
        for k in KEYS:
            assert g[1][k] == w[1][k], (i, k)
        assert np.ascontiguousarray(g[0]).tobytes() == np.ascontiguousarray(w[0]).tobytes(), i
        assert isinstance(g[1]["inliers"], torch.Tensor) and g[1]["inliers"].data_ptr() == mask[i].data_ptr()
        assert flags[i].tolist() == w[1]["inliers"], i
        kept = m[i][mask[i]]  # what one does next with a mask: index the match tensor, on the device
        assert kept.shape == (w[1]["num_inliers"], 5)
    # the single call: a uint8 mask, every second byte of a wider tensor
    pad = torch.full((N, 2), 9, dtype=torch.uint8, device="cuda")
    H, info = P.estimate_homography(clean[2, :, :2], clean[2, :, 2:4], opts[2], scores=m[2, :, 4], min_score=0.25, inliers_out=pad[:, 0])
    assert np.ascontiguousarray(H).tobytes() == np.ascontiguousarray(want[2][0]).tobytes()
    padded = pad.cpu().numpy()
    assert padded[:, 0].astype(bool).tolist() == want[2][1]["inliers"] and (padded[:, 1] == 9).all() and set(padded[:, 0]) <= {0, 1}
    H, info = P.estimate_homography(clean[2, :, :2], clean[2, :, 2:4], opts[2], inliers_out=mask[2])  # no scores
    plain = P.estimate_homography(u1[2], u2[2], opts[2])
    assert np.ascontiguousarray(H).tobytes() == np.ascontiguousarray(plain[0]).tobytes()
    assert mask[2].cpu().numpy().tolist() == plain[1]["inliers"] and info["n_used"] == N
    # what the binding cannot pass on
    for bad in (lambda: P.estimate_homography(u1[0], u2[0], opts[0], inliers_out=mask[0]),                     # host points
                lambda: P.estimate_homography(clean[0, :, :2], clean[0, :, 2:4], opts[0], inliers_out=mask[0, :100]),  # the wrong size
                lambda: P.estimate_homography(clean[0, :, :2], clean[0, :, 2:4], opts[0], inliers_out=mask[0].cpu()),  # a CPU tensor
                lambda: P.estimate_homography(clean[0, :, :2], clean[0, :, 2:4], opts[0], inliers_out=torch.zeros(N, device="cuda")),  # float
                lambda: P.undistort_points(OPENCV, m[0, :, :2], out=torch.zeros((N, 2), device="cuda")),       # a float32 destination
                lambda: P.undistort_points(OPENCV, m[0, :, :2], out=torch.zeros((N, 2), dtype=torch.float64)), # a CPU destination
                lambda: P.undistort_points_batch([(OPENCV, m[0, :, :2], None), (OPENCV, wide[0, :, :2], None)])):  # mixed
        try:
            bad()
            raise SystemExit("the binding passed on what it must refuse")
        except ValueError:
            pass
    print("torch device results child ok")


if __name__ == "__main__":
    main()
