#!/usr/bin/env python
"""ranked_points_bench.py - what ranking a matcher's confidences on the device costs, and what it replaces.

The workload is batch_device_bench.py's (BASELINE configs[4]: P3P / 5-point / homography cycling, N in [500, 5000], 30 - 70 %
outliers, default options, one call in flight) with one confidence per row: 1 on inliers, 0 on outliers, plus N(0, 0.35) noise,
rounded to float32; the rows of the padded (pairs, Nmax, 6) tensor behind a pair's matches carry NaN.  Every variant uses the
rows with score >= --min-score in descending score and PROSAC (ransac.progressive_sampling), so all three compute the same thing:

    (1) scored      float32 views of the tensor, scores = its column 5, through pl_estimate_batch_dev_scored
    (2) presorted   pl_estimate_batch_dev on a second tensor whose rows are sorted and compacted already - the parent commit's
                    capability; (1) - (2) is the price of ranking, permuted copy and mask scatter
    (3) round trip  what a C-ABI caller does without (1): copy the tensor to the host, sort every item there, pl_estimate_batch,
                    scatter the masks.  Its parts are timed separately; the sort is numpy per item, a C++ caller's would be
                    leaner, the copy and the call would not

After --warmup untimed rounds the variants alternate for --rounds rounds in one process; a timed step lies between two device
synchronisations.  (1) is checked equal to (2), item by item, bit by bit.  Then the ranking alone (rank_scores, which is launch,
synchronisation and read-back of the permutation: pl_debug_rank_scores, descriptors made once) at n = 512, 2048, 16384: one member per call, and 256 members in one grouped call.
One JSON line per measurement.

    python scripts/ranked_points_bench.py
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")  # one HIP stream per worker of the batch calls (see bench_batch.py)

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench_batch import make_problem  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, nargs="+", default=[4096, 512])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--streams", type=int, default=10, help="host threads inside the batch calls")
    ap.add_argument("--min-score", type=float, default=0.25)
    ap.add_argument("--rank-repeats", type=int, default=200)
    args = ap.parse_args()

    import torch  # (first: the library then shares torch's HIP runtime and knows the tensor's memory)

    import poselib_amd as P

    torch.cuda.set_device(0)
    P.set_device(0)

    total = max(args.problems)
    scenes = [make_problem(i) for i in range(total)]  # synthetic data, generated outside the timed region
    nmax = max(n for _, n, _ in scenes)
    padded = np.zeros((total, nmax, 6), dtype=np.float32)
    padded[:, :, 5] = np.nan
    rng = np.random.default_rng(1)
    for i, (kind, n, d) in enumerate(scenes):
        first, second = (d["p2d"], d["p3d"]) if kind == "abs" else (d["x1"], d["x2"])
        padded[i, :n, :2] = first
        padded[i, :n, 2:2 + second.shape[1]] = second
        padded[i, :n, 5] = d["inlier_gt"] + 0.35 * rng.standard_normal(n)
    orders = [P.score_order(padded[i, :, 5], args.min_score) for i in range(total)]
    sorted_rows = np.zeros_like(padded)
    for i, order in enumerate(orders):
        sorted_rows[i, :len(order)] = padded[i, order]
    tensor, tensor_sorted = torch.from_numpy(padded).cuda(), torch.from_numpy(sorted_rows).cuda()

    def problem(i, a, b, extra=None):
        kind, _, d = scenes[i]
        opt = dict({"ransac": {"seed": i, "progressive_sampling": True}}, **(extra or {}))
        if kind == "abs":
            return ("abs", a, b, d["camera"], opt)
        if kind == "rel":
            return ("rel", a, b, d["camera1"], d["camera2"], opt)
        return ("hom", a, b, opt)

    def cols(i):
        return 3 if scenes[i][0] == "abs" else 2

    def host_sorted(block, i):
        """what the caller of (3) does to item i of the block it copied back: rank, gather, widen"""
        order = P.score_order(block[i, :, 5], args.min_score)
        rows = block[i, order].astype(np.float64)
        return order, rows[:, :2], rows[:, 2:2 + cols(i)]

    for count in args.problems:
        scored = P.Batch([problem(i, tensor[i, :, :2], tensor[i, :, 2:2 + cols(i)], {"scores": tensor[i, :, 5], "min_score": args.min_score})
                          for i in range(count)])
        presorted = P.Batch([problem(i, tensor_sorted[i, :len(orders[i]), :2], tensor_sorted[i, :len(orders[i]), 2:2 + cols(i)])
                             for i in range(count)])
        assert scored.on_device and scored.scored and presorted.on_device and not presorted.scored
        state = {}

        def round_trip():
            t0 = time.perf_counter()
            block = tensor[:count].cpu().numpy()
            t1 = time.perf_counter()
            items = [host_sorted(block, i) for i in range(count)]
            t2 = time.perf_counter()
            batch = P.Batch([problem(i, a, b) for i, (_, a, b) in enumerate(items)])  # (marshalling: not part of the figure)
            t3 = time.perf_counter()
            batch.run(max_in_flight=args.streams)
            torch.cuda.synchronize()
            t4 = time.perf_counter()
            masks = []
            for (order, _, _), k in zip(items, batch.keep):
                mask = np.zeros(nmax, dtype=np.uint8)
                mask[order] = k[8][:len(order)]
                masks.append(mask)
            t5 = time.perf_counter()
            state["parts"] = {"copy_to_host": t1 - t0, "host_sort": t2 - t1, "pl_estimate_batch": t4 - t3, "mask_scatter": t5 - t4}
            return (t1 - t0) + (t2 - t1) + (t4 - t3) + (t5 - t4)

        variants = {"1_scored": lambda: scored.run(max_in_flight=args.streams), "2_presorted": lambda: presorted.run(max_in_flight=args.streams),
                    "3_round_trip": round_trip}
        times = {k: [] for k in variants}
        parts = {k: [] for k in ("copy_to_host", "host_sort", "pl_estimate_batch", "mask_scatter")}
        reports = {}
        names = list(variants)
        for rnd in range(args.warmup + args.rounds):
            for name in names[rnd % len(names):] + names[:rnd % len(names)]:  # (no variant always runs behind the same other one)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                own = variants[name]()
                torch.cuda.synchronize()
                dt = own if own is not None else time.perf_counter() - t0
                reports[name] = P.last_batch_report()
                if rnd >= args.warmup:
                    times[name].append(dt)
                    if name == "3_round_trip":
                        for k, v in state["parts"].items():
                            parts[k].append(v)
        mismatches = 0
        for i, ((ms, is_), (mp, ip)) in enumerate(zip(scored.results(), presorted.results())):
            same = all(is_[k] == ip[k] for k in ("refinements", "iterations", "num_inliers", "inlier_ratio", "model_score", "hypotheses"))
            mask = np.zeros(nmax, dtype=bool)
            mask[orders[i]] = ip["inliers"]
            blob = lambda m: (np.r_[m.pose.q, m.pose.t, m.camera.params] if hasattr(m, "pose") else  # noqa: E731
                              np.r_[m.q, m.t] if hasattr(m, "q") else np.ascontiguousarray(m)).tobytes()
            mismatches += int(not (same and is_["inliers"] == mask.tolist() and blob(ms) == blob(mp) and is_["n_used"] == len(orders[i])))
        out = {"workload": "batch_mixed (BASELINE configs[4]) + scores", "problems_per_call": count, "streams": args.streams,
               "rounds": args.rounds, "warmup": args.warmup, "min_score": args.min_score, "rows_per_item_mean": float(np.mean([s[1] for s in scenes[:count]])),
               "rows_used_mean": float(np.mean([len(o) for o in orders[:count]])), "items_1_not_equal_2": mismatches, "reports": reports}
        for name, ts in times.items():
            out[name] = {"ms_per_call_median": 1e3 * float(np.median(ts)), "min": 1e3 * min(ts), "max": 1e3 * max(ts),
                         "problems_per_s_median": count / float(np.median(ts))}
        out["3_round_trip"]["parts_ms_median"] = {k: 1e3 * float(np.median(v)) for k, v in parts.items()}
        out["price_of_ranking_ms"] = out["1_scored"]["ms_per_call_median"] - out["2_presorted"]["ms_per_call_median"]
        print(json.dumps(out), flush=True)
        if mismatches:
            raise SystemExit(f"{mismatches} items of the scored call differ from the call on the pre-sorted rows")

    # the ranking alone: the C call and nothing else (descriptors made once)
    from poselib_amd import _lib as L
    from poselib_amd import api

    def rank_call(members):
        cnt = len(members)
        desc, ns = (L.DeviceScores * cnt)(), (C.c_size_t * cnt)(*[int(m.shape[0]) for m in members])
        for k, m in enumerate(members):
            desc[k], _ = api._device_scores(m, ns[k], args.min_score)
        order, kept = np.zeros(sum(ns), dtype=np.uint32), (C.c_size_t * cnt)()
        ptr = order.ctypes.data_as(C.c_void_p)
        return (lambda: L.check(L.lib().pl_debug_rank_scores(desc, ns, C.c_size_t(cnt), ptr, kept))), order, kept

    def timed(fn, repeats):
        for _ in range(max(repeats // 10, 5)):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(repeats):
            fn()
        return (time.perf_counter() - t0) / repeats

    for n in (512, 2048, 16384):
        s = torch.from_numpy((rng.integers(0, 64, (256, n)) / 64.0).astype(np.float32)).cuda()
        want = P.score_order(s[3].cpu().numpy(), args.min_score)
        one, order, kept = rank_call([s[3]])
        single = timed(one, args.rank_repeats)
        assert order[:kept[0]].tolist() == want.tolist()
        many, _, _ = rank_call([s[k] for k in range(256)])
        grouped = timed(many, max(args.rank_repeats // 4, 5))
        print(json.dumps({"ranking_alone_n": n, "tile": P.rank_tile(n), "single_call_us": 1e6 * single, "grouped_256_members_call_us": 1e6 * grouped,
                          "grouped_us_per_member": 1e6 * grouped / 256,
                          "note": "pl_debug_rank_scores: checks, launch sequence, synchronisation, permutation read back"}), flush=True)

if __name__ == "__main__":
    main()
