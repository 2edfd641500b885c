"""Run by tests/test_gpu_batch_device_points.py in a process of its own: torch is imported BEFORE the product library, so both use
one HIP runtime.  The views of ONE padded (pairs, N, 4) float32 CUDA tensor - what a GPU matcher emits - go into estimate_batch
as they are and give the bits of the host call on the same values as doubles."""
import os
import sys

import torch  # first: see above

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import poselib_amd as P  # noqa: E402
from poselib_amd import synth  # noqa: E402

KEYS = ("refinements", "iterations", "num_inliers", "inlier_ratio", "model_score", "hypotheses", "inliers")
PAIRS, N = 8, 700


def main():
    if not torch.cuda.is_available():
        print("torch sees no GPU")
        return
    host = np.zeros((PAIRS, N, 4), dtype=np.float32)
    for i in range(PAIRS):
        h = synth.homography_scene(N, 0.3, 40 + i)
        host[i, :, :2], host[i, :, 2:] = h["x1"], h["x2"]
    t = torch.from_numpy(host).cuda()
    opts = [{"ransac": {"max_iterations": 2000, "min_iterations": 100, "seed": 7 + i}} for i in range(PAIRS)]
    wide = t.cpu().double().numpy()
    want = P.estimate_batch([("hom", wide[i, :, :2], wide[i, :, 2:], opts[i]) for i in range(PAIRS)])
    want_report = P.last_batch_report()
    views = [("hom", t[i, :, :2], t[i, :, 2:], opts[i]) for i in range(PAIRS)]
    assert views[3][1].stride(0) == 4 and views[3][2].storage_offset() == 3 * N * 4 + 2
    got = P.estimate_batch(views)
    assert P.last_batch_report() == want_report and want_report["grouped"] == PAIRS, (P.last_batch_report(), want_report)
    for i, (g, w) in enumerate(zip(got, want)):
        assert w[1]["num_inliers"] > 0.3 * N, i
        for k in KEYS:
            assert g[1][k] == w[1][k], (i, k)
        assert np.ascontiguousarray(g[0]).tobytes() == np.ascontiguousarray(w[0]).tobytes(), i
    for bad in (lambda: P.estimate_batch(views, devices=[0]),
                lambda: P.estimate_batch(views[:2] + [("hom", wide[2, :, :2], wide[2, :, 2:], opts[2])])):
        try:
            bad()
            raise SystemExit("a device batch took devices= or a host problem")
        except ValueError:
            pass
    print("torch batch child ok")


if __name__ == "__main__":
    main()
