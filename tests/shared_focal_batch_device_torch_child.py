"""Run by tests/test_gpu_shared_focal_batch_device.py in a process of its own: torch is imported BEFORE the product library, so both
use one HIP runtime.  A matcher's output as ONE padded (pairs, N, 5) float32 CUDA tensor - two views and a confidence per row, NaN
on the padding rows - goes into estimate_shared_focal_relative_pose_batch as views, scores = column 4, the masks into the rows of
one (pairs, N) torch.bool tensor.  Everything equals the host call on the ranked, widened rows; m[i][mask[i]] are its inliers."""
import os
import sys

import torch  # first: see above

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import poselib_amd as P  # noqa: E402
from poselib_amd import synth  # noqa: E402

KEYS = ("n_used", "refinements", "iterations", "num_inliers", "inlier_ratio", "model_score", "hypotheses")
PAIRS, N = 6, 320
MIN_SCORE = 0.25


def bits(model):
    return np.r_[model.pose.q, model.pose.t, model.camera1.params, model.camera2.params].tobytes()


def main():
    if not torch.cuda.is_available():
        print("torch sees no GPU")
        return
    rng = np.random.default_rng(21)
    host = np.zeros((PAIRS, N, 5), dtype=np.float32)
    rows = [N - 40 * (i % 3) for i in range(PAIRS)]  # the pairs' own lengths: the rest is padding
    pps, opts = [], []
    for i in range(PAIRS):
        pp = (500.0 + 4.5 * i, 490.0 - 2.25 * i)
        d = synth.relative_pose_scene(N, 0.3, 9300 + i, pp=pp)
        host[i, :, :2], host[i, :, 2:4] = d["x1"], d["x2"]
        host[i, :, 4] = np.round((d["inlier_gt"] + 0.4 * rng.standard_normal(N)) * 16) / 16
        host[i, rows[i]:, 4] = np.nan
        pps.append(list(pp))
        opts.append({"max_error": 2.0, "ransac": {"max_iterations": 1000, "min_iterations": 100, "seed": 4 + i}})
    m = torch.from_numpy(host).cuda()
    mask = torch.full((PAIRS, N), True, dtype=torch.bool, device="cuda")
    pairs = [(m[i, :, :2], m[i, :, 2:4], pps[i], dict(opts[i], scores=m[i, :, 4], min_score=MIN_SCORE, inliers_out=mask[i]))
             for i in range(PAIRS)]
    batch = P.SharedFocalBatch(pairs)
    batch.run(4)
    got = batch.results()
    report = P.last_batch_report()
    assert report == {"items": PAIRS, "grouped": 0, "focal_grouped": PAIRS, "solo": 0, "fallback": 0}, report
    back = mask.cpu().numpy()
    wide = host.astype(np.float64)
    for i in range(PAIRS):
        want = P.estimate_shared_focal_relative_pose(wide[i, :, :2], wide[i, :, 2:4], pps[i], opts[i], None, scores=host[i, :, 4],
                                                     min_score=MIN_SCORE)
        for k in KEYS:
            assert got[i][1][k] == want[1][k], (i, k, got[i][1][k], want[1][k])
        assert bits(got[i][0]) == bits(want[0]), i
        assert batch.n_used[i] == want[1]["n_used"] < rows[i]
        assert isinstance(got[i][1]["inliers"], torch.Tensor) and got[i][1]["inliers"].data_ptr() == mask[i].data_ptr()
        assert back[i].tolist() == want[1]["inliers"] and not back[i, rows[i]:].any(), i
        assert want[1]["num_inliers"] > 0.4 * want[1]["n_used"]
        chosen = m[i][mask[i]]  # what one does next: index the match tensor on the device
        assert chosen.shape == (want[1]["num_inliers"], 5)
        assert np.array_equal(chosen.cpu().numpy(), host[i][np.array(want[1]["inliers"])])
    # what the binding cannot pass on
    for bad in (lambda: P.SharedFocalBatch([(wide[0, :, :2], wide[0, :, 2:4], pps[0], opts[0])]),                  # host arrays
                lambda: P.SharedFocalBatch([(m[0, :, :2], wide[0, :, 2:4], pps[0], opts[0])]),                     # mixed sets
                lambda: P.SharedFocalBatch([(m[0, :, :2], m[0, :, 2:4], pps[0], dict(opts[0], scores=host[0, :, 4]))]),  # scores on the host
                lambda: P.SharedFocalBatch([(m[0, :, :2], m[0, :, 2:4], pps[0], dict(opts[0], inliers_out=mask[0].cpu()))])):  # a CPU tensor
        try:
            bad()
            raise SystemExit("the binding passed on what it must refuse")
        except ValueError:
            pass
    print("torch shared-focal batch child ok")


if __name__ == "__main__":
    main()
