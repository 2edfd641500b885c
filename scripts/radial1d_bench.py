#!/usr/bin/env python
"""Cost of the 1D-radial absolute-pose path next to plain absolute pose of the same build, on one scene shape
(synth.radial_1d_scene(5000, 0.5, seed) and the absolute_pose_scene it is made from).  Needs an MI355X; fails without one.

  * problems per second through pl_estimate_1D_radial_absolute_pose and pl_estimate_absolute_pose on the same scenes (host clock
    around calls that end in a device synchronise; the two alternate);
  * solo runs of the new kernels: `--kernels` runs the generator (pl_solve_batch kind 5 on 4096 samples), the streaming scorer
    (pl_debug_score_stream: 4096 hypotheses x 5000 correspondences) and k_lm<5> (pl_refine_model) a few times - run it under
    `rocprofv3 --kernel-trace --stats` for the kernel times, once more with POSELIB_AMD_NO_PREFILTER=1 for the scorer without the
    filter;
  * the share of non-inlier (hypothesis, correspondence) pairs that reach the exact pass with the filter on: `filter_share()` counts
    it on the host with the kernel's own predicate (tests/hostmath_radial1d) over 512 of `hypotheses()`; `--filter-share` prints that
    alone and needs no GPU.

Prints one JSON line per measurement.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MAX_ERROR = 2.0


def scenes(seed, n=5000, outl=0.5):
    from poselib_amd import synth

    return synth.radial_1d_scene(n, outl, seed), synth.absolute_pose_scene(n, outl, seed)


def front_scale(x):
    s = 0.0
    for k in range(x.shape[0]):
        s += float(np.sqrt(0.0 + x[k, 0] * x[k, 0] + x[k, 1] * x[k, 1]))
    return x.shape[0] / s


def hypotheses(d, H, seed):
    """the ground truth disturbed at every scale: a few good models among many bad ones, as a RANSAC batch holds them"""
    rs = np.random.RandomState(seed)
    M = np.zeros((H, 7))
    for k in range(H):
        s = 10.0 ** rs.uniform(-4, 0)
        q = np.asarray(d["q_gt"]) + s * rs.randn(4)
        M[k] = np.r_[q / np.linalg.norm(q), np.asarray(d["t_gt"])[:2] + s * rs.randn(2), 0.0]
    return M


def filter_share(count=512):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import hostmath_radial1d_lib as HR

    d, _ = scenes(1)
    scale = front_scale(d["p2d"])
    x = d["p2d"] * scale
    non_inlier = reach = inliers = 0
    for p in hypotheses(d, count, 2):
        st, rej, inl = HR.prefilter(p, x, d["p3d"], MAX_ERROR * scale)
        assert not (rej & inl).any()
        non_inlier += int((~inl).sum())
        reach += int((~inl & ~rej).sum())
        inliers += int(inl.sum())
    print(json.dumps({"what": "filter_share", "hypotheses": count, "non_inlier_pairs": non_inlier, "reach_exact_pass": reach,
                      "share": reach / max(non_inlier, 1), "inlier_pairs": inliers}))


def kernels(args):
    import poselib_amd as P

    d, _ = scenes(1)
    scale = front_scale(d["p2d"])
    x = d["p2d"] * scale
    thr = MAX_ERROR * scale
    M = hypotheses(d, args.hypotheses, 2)
    pr = P.Problem(P.KIND_RAD1D, x, d["p3d"])
    rs = np.random.RandomState(3)
    idx = np.array([rs.choice(x.shape[0], 5, replace=False) for _ in range(args.hypotheses)])
    first = np.concatenate([x[idx] / np.linalg.norm(x[idx], axis=2, keepdims=True), np.zeros(idx.shape + (1,))], axis=2)
    second = d["p3d"][idx]
    out = {}
    for _ in range(args.warmup):
        pr.score_stream(M, thr)
        P.solve_batch(P.KIND_RAD1D, first, second)
        pr.refine(P.CameraPose(M[1, :4], M[1, 4:]), {"loss_type": "TRUNCATED", "loss_scale": thr, "max_iterations": 25})
    t0 = time.perf_counter()
    for _ in range(args.steps):
        cnt, sc, path = pr.score_stream(M, thr)
    out["score_stream"] = {"call_ms": 1e3 * (time.perf_counter() - t0) / args.steps, "path": int(path), "best_count": int(cnt.max()),
                           "pairs": int(len(M) * pr.n)}
    t0 = time.perf_counter()
    for _ in range(args.steps):
        rec, n_models = P.solve_batch(P.KIND_RAD1D, first, second)
    out["solve_batch"] = {"call_ms": 1e3 * (time.perf_counter() - t0) / args.steps, "samples": int(len(first)), "models": int(n_models.sum())}
    t0 = time.perf_counter()
    for _ in range(args.steps):
        pose, it = pr.refine(P.CameraPose(M[1, :4], M[1, 4:]), {"loss_type": "TRUNCATED", "loss_scale": thr, "max_iterations": 25})
    out["refine"] = {"call_ms": 1e3 * (time.perf_counter() - t0) / args.steps, "iterations": int(it)}
    out["prefilter_off"] = bool(os.environ.get("POSELIB_AMD_NO_PREFILTER"))
    print(json.dumps({"what": "kernels", "hypotheses": args.hypotheses, **out}))


def throughput(args):
    import poselib_amd as P

    sc = [scenes(100 + k) for k in range(args.problems)]
    secs = {"radial1d": 0.0, "abs": 0.0}
    inl = {"radial1d": 0, "abs": 0}
    its = {"radial1d": 0, "abs": 0}
    for rep in range(args.warmup + args.steps):
        for which in ("abs", "radial1d"):
            t0 = time.perf_counter()
            for k, (r, a) in enumerate(sc):
                opt = {"max_error": MAX_ERROR, "ransac": {"seed": k}}
                if which == "abs":
                    _, info = P.estimate_absolute_pose(a["p2d"], a["p3d"], a["camera"], opt)
                else:
                    _, info = P.estimate_1D_radial_absolute_pose(r["p2d"], r["p3d"], opt)
                if rep == args.warmup:
                    inl[which] += info["num_inliers"]
                    its[which] += info["iterations"]
            if rep >= args.warmup:
                secs[which] += time.perf_counter() - t0
    for which in ("abs", "radial1d"):
        print(json.dumps({"what": "estimate", "estimator": which, "problems_per_s": args.problems * args.steps / secs[which],
                          "mean_inliers": inl[which] / args.problems, "mean_iterations": its[which] / args.problems,
                          "prefilter_off": bool(os.environ.get("POSELIB_AMD_NO_PREFILTER"))}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true", help="only the solo kernel runs (for a kernel trace)")
    ap.add_argument("--hypotheses", type=int, default=4096)
    ap.add_argument("--problems", type=int, default=16)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--filter-share", action="store_true", help="only the host-side count of pairs that pass the filter (no GPU)")
    args = ap.parse_args()
    if args.filter_share:
        filter_share()
        return
    import poselib_amd as P

    assert P.device_count() > 0, "no HIP device: this script measures on the GPU"
    kernels(args)
    if args.kernels:
        return
    throughput(args)
    filter_share()


if __name__ == "__main__":
    main()
