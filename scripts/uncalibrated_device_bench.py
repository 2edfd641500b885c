#!/usr/bin/env python
"""uncalibrated_device_bench.py - the two estimators of unknown cameras on a matcher's output that lives on the GPU
(profiles/uncalibrated_device_points.md).

For estimate_shared_focal_relative_pose and estimate_1D_radial_absolute_pose, on --rows correspondences at 30 % outliers held in
ONE float32 CUDA tensor (points and a confidence per row), the wall time of
  (a) device  the call on the tensor's column views with scores= and inliers_out= (a torch.bool tensor): nothing comes down
  (b) host    what a user did before: .cpu().numpy() of points and scores, score_order in numpy, the host entry point on the
              ranked rows, the mask scattered to the caller's numbering and copied back to the device
Each timed call lies between two device synchronisations; after --warmup untimed rounds the two variants alternate for --rounds
rounds in one process.  The results of (a) and (b) are checked equal.  --root: the tree whose poselib_amd is imported (another
checkout's, to time (b) on its host entry points; (a) is skipped where the package has no device form).  One JSON line per
measurement: median, min, max in milliseconds.

    python scripts/uncalibrated_device_bench.py
"""
import argparse
import inspect
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def report(name, times_ms, **extra):
    t = np.sort(np.array(times_ms))
    print(json.dumps(dict(name=name, median_ms=round(float(np.median(t)), 4), min_ms=round(float(t[0]), 4), max_ms=round(float(t[-1]), 4),
                          rounds=len(t), **extra)), flush=True)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--root", default=ROOT)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))

    import torch  # (first: the library then shares torch's HIP runtime and knows the tensors' memory)

    import poselib_amd as P
    from poselib_amd import synth

    assert torch.cuda.is_available(), "no GPU: nothing is measured"
    torch.cuda.set_device(0)
    P.set_device(0)
    sync = torch.cuda.synchronize
    N = args.rows
    rng = np.random.default_rng(3)
    opt = {"max_error": 2.0, "ransac": {"seed": 5}}

    d = synth.relative_pose_scene(N, 0.3, 8860)
    pp = list(d["camera1"]["params"][1:3])
    pair = np.zeros((N, 5), dtype=np.float32)
    pair[:, :2], pair[:, 2:4] = d["x1"], d["x2"]
    pair[:, 4] = d["inlier_gt"] + 0.35 * rng.standard_normal(N)
    r = synth.radial_1d_scene(N, 0.3, 8960)
    rad = np.zeros((N, 6), dtype=np.float32)
    rad[:, :2], rad[:, 2:5] = r["p2d"], r["p3d"]
    rad[:, 5] = pair[:, 4]
    cases = {"shared focal": (pair, (2, 4), 4, lambda a, b, **kw: P.estimate_shared_focal_relative_pose(a, b, pp, opt, None, **kw),
                              P.estimate_shared_focal_relative_pose),
             "1D radial": (rad, (2, 5), 5, lambda a, b, **kw: P.estimate_1D_radial_absolute_pose(a, b, opt, None, **kw),
                           P.estimate_1D_radial_absolute_pose)}
    for name, (host, cb, cs, fn, entry) in cases.items():
        m = torch.from_numpy(host).cuda()
        mask = torch.zeros(N, dtype=torch.bool, device="cuda")
        has_device_form = "inliers_out" in inspect.signature(entry).parameters
        out = {}

        def device():
            out["a"] = fn(m[:, 0:2], m[:, cb[0]:cb[1]], scores=m[:, cs], min_score=0.25, inliers_out=mask)

        def round_trip():
            h = m.cpu().numpy()
            order = P.score_order(h[:, cs], 0.25)
            a, b = h[:, 0:2].astype(np.float64)[order], h[:, cb[0]:cb[1]].astype(np.float64)[order]
            model, info = fn(a, b)
            flags = np.zeros(N, dtype=bool)
            flags[order] = info["inliers"]
            out["b"] = (model, info, torch.from_numpy(flags).cuda())

        variants = {"host": round_trip}
        if has_device_form:
            variants["device"] = device
        times = {k: [] for k in variants}
        for i in range(args.warmup + args.rounds):
            for k in (sorted(variants) if i % 2 == 0 else sorted(variants, reverse=True)):
                sync()
                t0 = time.perf_counter()
                variants[k]()
                sync()
                if i >= args.warmup:
                    times[k].append((time.perf_counter() - t0) * 1e3)
        med = {k: report(f"{name}: {k}", v, rows=N, iterations=out["b"][1]["iterations"], num_inliers=out["b"][1]["num_inliers"])
               for k, v in times.items()}
        if has_device_form:
            (ma, ia), (mb, ib, fb) = out["a"], out["b"]
            bits = lambda x: (np.r_[x.pose.q, x.pose.t, x.camera1.params] if hasattr(x, "camera1") else np.r_[x.q, x.t]).tobytes()
            equal = bits(ma) == bits(mb) and torch.equal(mask, fb) and all(ia[k] == ib[k] for k in ("iterations", "num_inliers", "model_score"))
            assert equal, f"{name}: the device call differs from the host round trip"
            print(json.dumps(dict(name=f"{name}: ratio", host_over_device=round(med["host"] / med["device"], 3), equal=equal)), flush=True)


if __name__ == "__main__":
    main()
