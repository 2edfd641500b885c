"""Host-input against device-input calls of the same problem (profiles/device_points.md).

    python scripts/device_points_bench.py [--reps 15] [--json FILE]

One front-end per kind (absolute pose, relative pose, fundamental, homography) and the creation of a resident problem, at
n = 2000 and n = 16384, points in fp64 and fp32.  The host call gets its float64 arrays ready in host memory (for fp32: the widened
values) - a caller whose matches are on the GPU pays the copy to the host and the widening on top, which is not timed here.  The
device call gets arrays that already lie in device memory.  Medians of wall time over `--reps` calls after two warm-up calls.
k_point_stats: wall time of one launch and its wait, through the diagnostic entry (two launches per call) on fp64 points read in
place."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import poselib_amd as P  # noqa: E402
from device_arrays import on_gpu  # noqa: E402
from poselib_amd import synth  # noqa: E402


def median_ms(fn, reps):
    for _ in range(2):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t)


def cases(n):
    d = synth.absolute_pose_scene(n, 0.3, 1)
    yield "estimate_absolute_pose", d["p2d"], d["p3d"], lambda a, b, d=d: P.estimate_absolute_pose(a, b, d["camera"], {"ransac": {"seed": 1}})
    d = synth.relative_pose_scene(n, 0.3, 2)
    yield "estimate_relative_pose", d["x1"], d["x2"], lambda a, b, d=d: P.estimate_relative_pose(a, b, d["camera1"], d["camera2"], {"ransac": {"seed": 1}})
    d = synth.fundamental_scene(n, 0.3, 3)
    yield "estimate_fundamental", d["x1"], d["x2"], lambda a, b: P.estimate_fundamental(a, b, {"ransac": {"seed": 1}})
    d = synth.homography_scene(n, 0.3, 4)
    yield "estimate_homography", d["x1"], d["x2"], lambda a, b: P.estimate_homography(a, b, {"ransac": {"seed": 1}})
    yield "Problem(KIND_HOM) creation", d["x1"], d["x2"], lambda a, b: P.Problem(P.KIND_HOM, a, b).close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--json")
    args = ap.parse_args()
    rows = []
    for n in (2000, 16384):
        for name, a, b, call in cases(n):
            for dtype in (np.float64, np.float32):
                ha, hb = a.astype(dtype).astype(np.float64), b.astype(dtype).astype(np.float64)
                da, db = on_gpu(a, dtype), on_gpu(b, dtype)
                host = median_ms(lambda: call(ha, hb), args.reps)
                dev = median_ms(lambda: call(da, db), args.reps)
                rows.append({"case": name, "n": n, "dtype": np.dtype(dtype).name, "host_ms": host, "device_ms": dev})
                print(f"{name:28s} n={n:6d} {np.dtype(dtype).name}: host input {host:8.3f} ms, device input {dev:8.3f} ms", flush=True)
        d = synth.fundamental_scene(n, 0.3, 3)
        da, db = on_gpu(d["x1"]), on_gpu(d["x2"])
        ms = median_ms(lambda: P.point_stats_dev(da, db, True), args.reps) / 2
        rows.append({"case": "k_point_stats (launch + wait)", "n": n, "dtype": "float64", "device_ms": ms})
        print(f"{'k_point_stats (launch + wait)':28s} n={n:6d}: {ms:8.3f} ms", flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
