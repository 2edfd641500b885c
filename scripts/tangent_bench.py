#!/usr/bin/env python
"""Cost of the tangent-Sampson relative-pose path next to the plain path of the same build, on bench.py's config-2 shape
(synth.relative_pose_scene(5000, 0.5, seed)).  Needs an MI355X; fails without one.

  * problems per second through pl_estimate_relative_pose with and without `tangent_sampson` (host clock around calls that end in a
    device synchronise; the two alternate);
  * solo time of the streaming scorers on a fixed list of hypotheses: `--kernels` runs pl_debug_score_stream on an EST_RELT and on an
    EST_REL problem of the same scene (run it under `rocprofv3 --kernel-trace --stats` for the kernel times);
  * the share of non-inlier (hypothesis, correspondence) pairs that reach the exact pass with the filter on: `filter_share()` counts
    it on the host with the kernel's own predicate (tests/hostmath_tangent: pf_tangent_point / pf_tangent_outlier compiled for the
    host) over 512 of `hypotheses()`; `--filter-share` prints that alone and needs no GPU;
  * the device-side view of the filter: every measurement once more in a fresh process with POSELIB_AMD_NO_PREFILTER=1.

Prints one JSON line per measurement.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def scene(seed, n=5000, outl=0.5):
    from poselib_amd import synth

    return synth.relative_pose_scene(n, outl, seed)


def hypotheses(d, H, seed):
    """the ground truth disturbed at every scale: a few good models among many bad ones, as a RANSAC batch holds them"""
    rs = np.random.RandomState(seed)
    M = np.zeros((H, 7))
    for k in range(H):
        s = 10.0 ** rs.uniform(-4, 0)
        q = np.asarray(d["q_gt"]) + s * rs.randn(4)
        M[k] = np.r_[q / np.linalg.norm(q), np.asarray(d["t_gt"]) + s * rs.randn(3)]
    return M


def filter_share(count=512):
    """non-inlier pairs (r^2 >= thr^2 in exact fp64) of the benchmark scene that the fp32 pre-filter of k_score_tangent lets through"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import hostmath_tangent_lib as HT

    d = scene(1)
    f, cx, cy = d["camera1"]["params"]
    cam = {"model": 0, "params": [1.0, cx / f, cy / f]}
    d1, M1, _ = HT.unproject_with_jac(cam, np.asarray(d["x1"]) / f)
    d2, M2, _ = HT.unproject_with_jac(cam, np.asarray(d["x2"]) / f)
    non_inlier = reach = below_thr = 0
    for p in hypotheses(d, count, 2):
        w, x, y, z = p[:4]
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                      [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                      [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
        t = p[4:]
        E = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]) @ R
        st, rej, below, _ = HT.prefilter(E, d1, d2, M1, M2, 1.0 / f)
        assert not (rej & below).any()
        non_inlier += int((~below).sum())
        reach += int((~below & ~rej).sum())
        below_thr += int(below.sum())
    print(json.dumps({"what": "filter_share", "hypotheses": count, "non_inlier_pairs": non_inlier, "reach_exact_pass": reach,
                      "share": reach / max(non_inlier, 1), "pairs_below_threshold": below_thr}))


def kernels(args):
    import poselib_amd as P

    d = scene(1)
    f, cx, cy = d["camera1"]["params"]
    M = hypotheses(d, args.hypotheses, 2)
    scale = 1.0 / f
    cam = {"model": 0, "params": [f * scale, cx * scale, cy * scale]}
    pt = P.TangentProblem(np.asarray(d["x1"]) * scale, np.asarray(d["x2"]) * scale, cam, cam)
    pr = P.Problem(P.KIND_REL, (np.asarray(d["x1"]) - [cx, cy]) / f, (np.asarray(d["x2"]) - [cx, cy]) / f)
    thr = 1.0 / f
    out = {}
    for name, prob in (("tangent", pt), ("plain", pr)):
        for _ in range(args.warmup):
            prob.score_stream(M, thr)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            cnt, sc, path = prob.score_stream(M, thr)
        out[name] = {"call_ms": 1e3 * (time.perf_counter() - t0) / args.steps, "path": int(path), "best_count": int(cnt.max()),
                     "pairs": int(len(M) * prob.n)}
    out["prefilter_off"] = bool(os.environ.get("POSELIB_AMD_NO_PREFILTER"))
    print(json.dumps({"what": "score_stream", "hypotheses": args.hypotheses, **out}))


def throughput(args):
    import poselib_amd as P

    scenes = [scene(100 + k) for k in range(args.problems)]
    opts = {False: {"max_error": 1.0}, True: {"max_error": 1.0, "tangent_sampson": True}}
    secs = {False: 0.0, True: 0.0}
    inl = {False: 0, True: 0}
    its = {False: 0, True: 0}
    for rep in range(args.warmup + args.steps):
        for flag in (False, True):
            t0 = time.perf_counter()
            for k, d in enumerate(scenes):
                _, info = P.estimate_relative_pose(d["x1"], d["x2"], d["camera1"], d["camera2"], dict(opts[flag], ransac={"seed": k}))
                if rep == args.warmup:
                    inl[flag] += info["num_inliers"]
                    its[flag] += info["iterations"]
            if rep >= args.warmup:
                secs[flag] += time.perf_counter() - t0
    for flag in (False, True):
        print(json.dumps({"what": "estimate_relative_pose", "tangent_sampson": flag, "problems_per_s": args.problems * args.steps / secs[flag],
                          "mean_inliers": inl[flag] / args.problems, "mean_iterations": its[flag] / args.problems,
                          "prefilter_off": bool(os.environ.get("POSELIB_AMD_NO_PREFILTER"))}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true", help="only the pl_debug_score_stream calls (for a kernel trace)")
    ap.add_argument("--hypotheses", type=int, default=4096)
    ap.add_argument("--problems", type=int, default=16)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--child", action="store_true")
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
    if not args.child:
        filter_share()
    if not args.child and not os.environ.get("POSELIB_AMD_NO_PREFILTER"):  # the same without the filter, in a fresh process
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--hypotheses", str(args.hypotheses), "--problems",
                            str(args.problems), "--steps", str(args.steps), "--warmup", str(args.warmup)],
                           env=dict(os.environ, POSELIB_AMD_NO_PREFILTER="1"), capture_output=True, text=True, timeout=600)
        sys.stdout.write(r.stdout)
        assert r.returncode == 0, r.stderr


if __name__ == "__main__":
    main()
