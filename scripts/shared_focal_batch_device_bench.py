#!/usr/bin/env python
"""shared_focal_batch_device_bench.py - batches of shared-focal pairs on a matcher's output that lives on the GPU
(profiles/shared_focal_batch_device.md).

--pairs pairs of --rows correspondences at 30 % outliers in ONE float32 CUDA tensor (pairs, rows, 5) - two views and a confidence
per row, min_score 0.25 - the masks in one (pairs, rows) torch.bool tensor.  The wall time of
  (a) batch   estimate_shared_focal_relative_pose_batch's call on the tensor's views, marshalled once (SharedFocalBatch.run())
  (b) host    what a user did before for the batch rate: .cpu().numpy(), score_order in numpy per pair, the host estimate_batch
              with "shared_focal" problems on the ranked rows, the masks scattered to the caller's numbering and copied back
  (c) loop    the loop of single device calls (estimate_shared_focal_relative_pose with scores= and inliers_out=)
Each timed call lies between two device synchronisations; after --warmup untimed rounds the variants alternate for --rounds
rounds in one process.  The results of (a), (b) and (c) are checked equal.  --root: the tree whose poselib_amd is imported (another
checkout's, to time (b) and (c) there; (a) is skipped where the package has no batch form).  One JSON line per measurement:
median, min, max in milliseconds and pairs per second.

    python scripts/shared_focal_batch_device_bench.py
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def report(name, times_ms, pairs, **extra):
    t = np.sort(np.array(times_ms))
    med = float(np.median(t))
    print(json.dumps(dict(name=name, median_ms=round(med, 3), min_ms=round(float(t[0]), 3), max_ms=round(float(t[-1]), 3),
                          pairs_per_s=round(pairs / (med * 1e-3), 1), rounds=len(t), **extra)), flush=True)
    return med, float(t[-1] - t[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=512)
    ap.add_argument("--rows", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--max-in-flight", type=int, default=8)
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
    K, N, MIN = args.pairs, args.rows, 0.25
    rng = np.random.default_rng(3)
    host = np.zeros((K, N, 5), dtype=np.float32)
    pps, opts = [], []
    for i in range(K):
        pp = (500.0 + 0.25 * (i % 64), 500.0 - 0.5 * (i % 32))
        d = synth.relative_pose_scene(N, 0.3, 20000 + i, pp=pp)
        host[i, :, :2], host[i, :, 2:4] = d["x1"], d["x2"]
        host[i, :, 4] = d["inlier_gt"] + 0.35 * rng.standard_normal(N)
        pps.append(list(pp))
        opts.append({"max_error": 2.0, "ransac": {"seed": 5 + i}})
    m = torch.from_numpy(host).cuda()
    has_batch_form = hasattr(P, "SharedFocalBatch")
    masks = {k: torch.zeros((K, N), dtype=torch.bool, device="cuda") for k in "abc"}
    out = {}

    if has_batch_form:
        batch = P.SharedFocalBatch([(m[i, :, :2], m[i, :, 2:4], pps[i], dict(opts[i], scores=m[i, :, 4], min_score=MIN, inliers_out=masks["a"][i]))
                                    for i in range(K)])

    def run_batch():
        batch.run(args.max_in_flight)
        out["a"] = batch

    def round_trip():
        h = m.cpu().numpy()
        orders = [P.score_order(h[i, :, 4], MIN) for i in range(K)]
        wide = h[:, :, :4].astype(np.float64)
        res = P.estimate_batch([("shared_focal", wide[i, orders[i], :2], wide[i, orders[i], 2:4], pps[i], opts[i]) for i in range(K)],
                               args.max_in_flight)
        flags = np.zeros((K, N), dtype=bool)
        for i in range(K):
            flags[i, orders[i]] = res[i][1]["inliers"]
        masks["b"].copy_(torch.from_numpy(flags))
        out["b"] = res

    def loop():
        out["c"] = [P.estimate_shared_focal_relative_pose(m[i, :, :2], m[i, :, 2:4], pps[i], opts[i], None, scores=m[i, :, 4], min_score=MIN,
                                                          inliers_out=masks["c"][i]) for i in range(K)]

    variants = {"b host round trip": round_trip, "c loop of single device calls": loop}
    if has_batch_form:
        variants["a batch from device memory"] = run_batch
    times = {k: [] for k in variants}
    for r in range(args.warmup + args.rounds):
        for k in (sorted(variants) if r % 2 == 0 else sorted(variants, reverse=True)):
            sync()
            t0 = time.perf_counter()
            variants[k]()
            sync()
            if r >= args.warmup:
                times[k].append((time.perf_counter() - t0) * 1e3)
    stats = {k[0]: report(k, v, K, rows=N, root=os.path.abspath(args.root)) for k, v in times.items()}

    bits = lambda x: np.r_[x.pose.q, x.pose.t, x.camera1.params].tobytes()  # noqa: E731
    keys = ("iterations", "refinements", "num_inliers", "model_score", "n_used")
    rb, rc = out["b"], out["c"]
    equal = torch.equal(masks["b"], masks["c"]) and all(bits(rb[i][0]) == bits(rc[i][0]) for i in range(K))
    equal = equal and all(rb[i][1][k] == rc[i][1][k] for i in range(K) for k in keys)
    if has_batch_form:
        ra = out["a"].results()
        equal = equal and torch.equal(masks["a"], masks["b"]) and all(bits(ra[i][0]) == bits(rb[i][0]) for i in range(K))
        equal = equal and all(ra[i][1][k] == rb[i][1][k] for i in range(K) for k in keys)
        run_batch()
        print(json.dumps(dict(name="a last_batch_report", **P.last_batch_report())), flush=True)
    assert equal, "the variants' results differ"
    solved = int(sum(r[1]["num_inliers"] > 0.4 * r[1]["n_used"] for r in rb))
    summary = dict(name="summary", equal=equal, pairs=K, rows=N, solved=solved,
                   mean_iterations=round(float(np.mean([r[1]["iterations"] for r in rb])), 1))
    if has_batch_form:
        (ma, _), (mb, spread_b), (mc, _) = stats["a"], stats["b"], stats["c"]
        summary.update(a_over_b=round(ma / mb, 3), b_spread_ms=round(spread_b, 3), a_not_above_b_by_more_than_its_spread=bool(ma <= mb + spread_b),
                       c_over_a=round(mc / ma, 2))
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
