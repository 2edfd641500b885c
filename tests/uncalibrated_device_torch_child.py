"""Run by tests/test_gpu_uncalibrated_device_points.py in a process of its own: torch is imported BEFORE the product library, so both
use one HIP runtime.  A matcher's output as ONE padded (pairs, N, 5) float32 CUDA tensor - two views and a confidence per row -
goes into estimate_shared_focal_relative_pose, a (N, 6) tensor of pixels, 3-D points and confidences into
estimate_1D_radial_absolute_pose; the masks land in a torch.bool row of a (3, N) tensor and in a uint8 column of a wider one whose
other elements keep their 0xAB.  Everything equals the numpy path on the widened values."""
import os
import sys

import torch  # first: see above

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import poselib_amd as P  # noqa: E402
from poselib_amd import synth  # noqa: E402

KEYS = ("n_used", "refinements", "iterations", "num_inliers", "inlier_ratio", "model_score", "hypotheses")
N = 300
FILL = 0xAB


def bits(model):
    if hasattr(model, "camera1"):
        return np.r_[model.pose.q, model.pose.t, model.camera1.params, model.camera2.params].tobytes()
    return np.r_[model.q, model.t].tobytes()


def same(got, want, what):
    for k in KEYS:
        assert got[1][k] == want[1][k], (what, k, got[1][k], want[1][k])
    assert bits(got[0]) == bits(want[0]), what


def main():
    if not torch.cuda.is_available():
        print("torch sees no GPU")
        return
    rng = np.random.default_rng(12)
    opt = {"max_error": 2.0, "ransac": {"max_iterations": 1000, "min_iterations": 100, "seed": 4}}
    d = synth.relative_pose_scene(N, 0.3, 8850)
    pp = list(d["camera1"]["params"][1:3])
    pair = np.zeros((N, 5), dtype=np.float32)
    pair[:, :2], pair[:, 2:4] = d["x1"], d["x2"]
    pair[:, 4] = np.round((d["inlier_gt"] + 0.4 * rng.standard_normal(N)) * 16) / 16
    pair[N - 30:, 4] = np.nan  # padding rows
    r = synth.radial_1d_scene(N, 0.3, 8950)
    rad = np.zeros((N, 6), dtype=np.float32)
    rad[:, :2], rad[:, 2:5] = r["p2d"], r["p3d"]
    rad[:, 5] = pair[:, 4]
    cases = {"sfocal": (pair, lambda a, b, **kw: P.estimate_shared_focal_relative_pose(a, b, pp, opt, None, **kw), (0, 2), (2, 4), 4),
             "radial": (rad, lambda a, b, **kw: P.estimate_1D_radial_absolute_pose(a, b, opt, None, **kw), (0, 2), (2, 5), 5)}
    for kind, (host, fn, ca, cb, cs) in cases.items():
        wide = host.astype(np.float64)
        m = torch.from_numpy(host).cuda()
        a, b, s = m[:, ca[0]:ca[1]], m[:, cb[0]:cb[1]], m[:, cs]
        wa, wb = wide[:, ca[0]:ca[1]], wide[:, cb[0]:cb[1]]
        # plain: device against host
        want = fn(wa, wb)
        got = fn(a, b)
        same(got, want, (kind, "plain"))
        assert got[1]["inliers"] == want[1]["inliers"] and want[1]["num_inliers"] > 0.4 * N
        # scores and a mask in device memory: a torch.bool row of a (3, N) tensor
        want = fn(wa, wb, scores=host[:, cs], min_score=0.25)
        rows = torch.full((3, N), True, dtype=torch.bool, device="cuda")
        got = fn(a, b, scores=s, min_score=0.25, inliers_out=rows[1])
        same(got, want, (kind, "scored, bool row"))
        assert isinstance(got[1]["inliers"], torch.Tensor) and got[1]["inliers"].data_ptr() == rows[1].data_ptr()
        back = rows.cpu().numpy()
        assert back[1].tolist() == want[1]["inliers"] and back[0].all() and back[2].all(), kind
        assert m[rows[1]].shape == (want[1]["num_inliers"], host.shape[1])  # what one does next: index the match tensor on the device
        # ... and a uint8 column of a wider block, without scores
        want = fn(wa, wb)
        block = torch.full((N, 4), FILL, dtype=torch.uint8, device="cuda")
        got = fn(a, b, inliers_out=block[:, 2])
        same(got, want, (kind, "plain, uint8 column"))
        back = block.cpu().numpy()
        assert back[:, 2].astype(bool).tolist() == want[1]["inliers"] and set(back[:, 2]) <= {0, 1}
        assert (np.delete(back, 2, axis=1) == FILL).all(), kind
        # what the binding cannot pass on
        for bad in (lambda: fn(wa, b),                                  # host and device points mixed
                    lambda: fn(wa, wb, inliers_out=rows[1]),            # a device mask with host points
                    lambda: fn(a, b, scores=host[:, cs]),               # scores on the host, points on the device
                    lambda: fn(a, b, inliers_out=rows[1].cpu())):       # a CPU tensor
            try:
                bad()
                raise SystemExit("the binding passed on what it must refuse")
            except ValueError:
                pass
    print("torch uncalibrated child ok")


if __name__ == "__main__":
    main()
