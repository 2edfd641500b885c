"""Run by tests/test_gpu_ranked_points.py in a process of its own: torch is imported BEFORE the product library, so both use one HIP
runtime.  ONE padded (pairs, N, 5) float32 CUDA tensor - matches and their confidence, what a GPU matcher emits - goes into
estimate_batch as views: columns 0:2 and 2:4 are the points, column 4 the scores (stride 5).  Every item gives the bits of the host
call on the kept rows in ranked order, as doubles."""
import os
import sys

import torch  # first: see above

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import poselib_amd as P  # noqa: E402
from poselib_amd import synth  # noqa: E402

KEYS = ("refinements", "iterations", "num_inliers", "inlier_ratio", "model_score", "hypotheses")
PAIRS, N = 6, 500


def main():
    if not torch.cuda.is_available():
        print("torch sees no GPU")
        return
    host = np.zeros((PAIRS, N, 5), dtype=np.float32)
    rng = np.random.default_rng(3)
    for i in range(PAIRS):
        h = synth.homography_scene(N, 0.4, 60 + i)
        host[i, :, :2], host[i, :, 2:4] = h["x1"], h["x2"]
        host[i, :, 4] = np.round((h["inlier_gt"] + 0.4 * rng.standard_normal(N)) * 16) / 16
        host[i, N - 40 * i:, 4] = np.nan  # padding rows, another number per pair
    t = torch.from_numpy(host).cuda()
    opts = [{"ransac": {"max_iterations": 2000, "min_iterations": 100, "seed": 7 + i, "progressive_sampling": True}} for i in range(PAIRS)]
    wide = host.astype(np.float64)
    orders = [P.score_order(host[i, :, 4], 0.25) for i in range(PAIRS)]
    want = P.estimate_batch([("hom", wide[i, orders[i], :2], wide[i, orders[i], 2:4], opts[i]) for i in range(PAIRS)])
    want_report = P.last_batch_report()
    views = [("hom", t[i, :, :2], t[i, :, 2:4], dict(opts[i], scores=t[i, :, 4], min_score=0.25)) for i in range(PAIRS)]
    assert views[3][3]["scores"].stride(0) == 5 and views[3][3]["scores"].storage_offset() == 3 * N * 5 + 4
    got = P.estimate_batch(views)
    assert P.last_batch_report() == want_report and want_report["grouped"] == PAIRS, (P.last_batch_report(), want_report)
    for i, (g, w) in enumerate(zip(got, want)):
        assert w[1]["num_inliers"] > 0.3 * len(orders[i]), i
        for k in KEYS:
            assert g[1][k] == w[1][k], (i, k)
        mask = np.zeros(N, dtype=bool)
        mask[orders[i]] = w[1]["inliers"]
        assert g[1]["inliers"] == mask.tolist() and g[1]["n_used"] == len(orders[i]), i
        assert np.ascontiguousarray(g[0]).tobytes() == np.ascontiguousarray(w[0]).tobytes(), i
    # the single call, and the permutation itself, from the same column
    H, info = P.estimate_homography(t[2, :, :2], t[2, :, 2:4], opts[2], scores=t[2, :, 4], min_score=0.25)
    assert np.ascontiguousarray(H).tobytes() == np.ascontiguousarray(got[2][0]).tobytes() and info["inliers"] == got[2][1]["inliers"]
    assert P.rank_scores(t[2, :, 4], 0.25).tolist() == orders[2].tolist()
    try:
        P.estimate_homography(t[2, :, :2], t[2, :, 2:4], opts[2], scores=host[2, :, 4])
        raise SystemExit("device points took host scores")
    except ValueError:
        pass
    print("torch ranked child ok")


if __name__ == "__main__":
    main()
