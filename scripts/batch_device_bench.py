#!/usr/bin/env python
"""batch_device_bench.py - what pl_estimate_batch_dev gains over pl_estimate_batch when the matches are on the GPU already.

The workload is bench_batch.py's (BASELINE configs[4]: P3P / 5-point / homography cycling, N in [500, 5000], 30 - 70 % outliers,
default options), one call in flight, at --problems per call (default 4096 and 512).  The correspondences are rounded to float32
once - a matcher's output - and every variant works on those values:

    (a) host arrays (float64) through pl_estimate_batch of ANOTHER build of the library (--parent-lib: the parent commit's)
    (b) host arrays (float64) through pl_estimate_batch of this build
    (c) float32 views of ONE padded (pairs, Nmax, 5) device tensor through pl_estimate_batch_dev of this build

After --warmup untimed rounds the variants alternate for --rounds rounds inside one process (a, b, c, then b, c, a, ...: the
order rotates, so that no variant always follows the same other one); a timed step is
the C-ABI call and nothing else, between two device synchronisations.  (c)'s results are checked equal to (b)'s, item by item, bit
by bit.  One JSON line per call size: problems/s per variant (median, min, max over the rounds); the spread of (b) is the
yardstick for "(a) and (b) do not differ".  POSELIB_AMD_GROUP_TIMING=1 in the environment makes the library print where the
workers' time went (stage A among the phases) on stderr, call by call; the timed figures of such a run are not the ones to quote.

    python scripts/batch_device_bench.py --parent-lib /path/to/parent/libposelib_amd.so
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
    ap.add_argument("--warmup", type=int, default=3, help="untimed rounds (the workers' device arenas grow during the first two)")
    ap.add_argument("--streams", type=int, default=10, help="host threads inside the batch calls")
    ap.add_argument("--parent-lib", default=None, help="a libposelib_amd.so of the parent commit: variant (a)")
    args = ap.parse_args()

    import torch  # (first: the library then shares torch's HIP runtime and knows the tensor's memory)

    import poselib_amd as P
    from poselib_amd import _lib as L

    torch.cuda.set_device(0)
    P.set_device(0)
    parent = None
    if args.parent_lib:
        assert os.path.realpath(args.parent_lib) != os.path.realpath(P.LIB_PATH), "--parent-lib is this build"
        L.lib()
        parent = C.CDLL(args.parent_lib)
        parent.pl_estimate_batch.restype = C.c_int
        parent.pl_estimate_batch.argtypes = [C.POINTER(L.BatchItem), C.c_size_t, C.c_int]
        assert parent.pl_abi_version() == L.ABI_VERSION

    total = max(args.problems)
    scenes = [make_problem(i) for i in range(total)]  # synthetic data, generated outside the timed region
    nmax = max(n for _, n, _ in scenes)
    padded = np.zeros((total, nmax, 5), dtype=np.float32)
    for i, (kind, n, d) in enumerate(scenes):
        first, second = (d["p2d"], d["p3d"]) if kind == "abs" else (d["x1"], d["x2"])
        padded[i, :n, :2] = first
        padded[i, :n, 2:2 + second.shape[1]] = second
    tensor = torch.from_numpy(padded).cuda()

    def problem(i, device):
        kind, n, d = scenes[i]
        src = tensor if device else padded
        cols = 3 if kind == "abs" else 2
        a, b = src[i, :n, :2], src[i, :n, 2:2 + cols]
        if not device:
            a, b = a.astype(np.float64), b.astype(np.float64)  # (exact: the values of the float32 tensor)
        opt = {"ransac": {"seed": i}}
        if kind == "abs":
            return ("abs", a, b, d["camera"], opt)
        if kind == "rel":
            return ("rel", a, b, d["camera1"], d["camera2"], opt)
        return ("hom", a, b, opt)

    for count in args.problems:
        host = P.Batch([problem(i, False) for i in range(count)])
        dev = P.Batch([problem(i, True) for i in range(count)])
        assert dev.on_device and not host.on_device
        variants = {"b_host": lambda: host.run(max_in_flight=args.streams), "c_device": lambda: dev.run(max_in_flight=args.streams)}
        if parent is not None:
            variants = dict(a_parent_host=lambda: L.check(parent.pl_estimate_batch(host.items, C.c_size_t(count), C.c_int(args.streams))),
                            **variants)
        times = {k: [] for k in variants}
        reports = {}
        names = list(variants)
        for rnd in range(args.warmup + args.rounds):
            for name in names[rnd % len(names):] + names[:rnd % len(names)]:  # (no variant always runs behind the same other one)
                run = variants[name]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if rnd >= args.warmup:
                    times[name].append(dt)
                if name != "a_parent_host":
                    reports[name] = P.last_batch_report()
        # (c) equals (b): stats, masks and models of every item (both batches hold the results of their last run)
        mismatches = 0
        for (mh, ih), (md, idv) in zip(host.results(), dev.results()):
            same = all(ih[k] == idv[k] for k in ("refinements", "iterations", "num_inliers", "inlier_ratio", "model_score", "hypotheses",
                                                 "inliers"))
            blob = lambda m: (np.r_[m.pose.q, m.pose.t, m.camera.params] if hasattr(m, "pose") else  # noqa: E731
                              np.r_[m.q, m.t] if hasattr(m, "q") else np.ascontiguousarray(m)).tobytes()
            mismatches += int(not (same and blob(mh) == blob(md)))
        out = {"workload": "batch_mixed (BASELINE configs[4])", "problems_per_call": count, "calls_in_flight": 1, "streams": args.streams,
               "rounds": args.rounds, "warmup": args.warmup, "items_c_not_equal_b": mismatches, "reports": reports,
               "group_timing": bool(os.environ.get("POSELIB_AMD_GROUP_TIMING"))}
        for name, ts in times.items():
            rate = sorted(count / t for t in ts)
            out[name] = {"problems_per_s_median": float(np.median(rate)), "min": rate[0], "max": rate[-1],
                         "ms_per_call_median": 1e3 * float(np.median(ts))}
        print(json.dumps(out), flush=True)
        if mismatches:
            raise SystemExit(f"{mismatches} items of the device call differ from the host call")


if __name__ == "__main__":
    main()
