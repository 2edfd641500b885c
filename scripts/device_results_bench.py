#!/usr/bin/env python
"""device_results_bench.py - what keeping the results on the device saves (profiles/device_results.md).

(a) Undistortion.  64 views x 10 000 points, OPENCV camera, resident float32 tensors (the two point columns of a matcher's
    (views, N, 4) tensor).
      dev         pl_undistort_points_batch_dev into a preallocated float64 (views, N, 2) tensor: one call for all views; the
                  descriptors are made once, the timed step is the library call
      python      the same through poselib_amd.undistort_points_batch (descriptors and stream synchronisation every call)
      round trip  what the parent commit offers for tensors: per view tensor -> host (float64) -> pl_undistort_points -> tensor
    dev is checked equal to round trip, bit for bit.
(b) Masks.  estimate_batch on 512 homography pairs x 2048 rows with scores (float32 (pairs, N, 5) tensor, 30 % outliers, PROSAC off,
    default options otherwise), followed by m[i][mask[i]] on the device for every pair.
      device masks   "inliers_out": mask[i], a (pairs, N) torch.bool tensor - pl_estimate_batch_dev_masked
      host masks     the parent's call (pl_estimate_batch_dev_scored): info["inliers"] is a list, uploaded again for the indexing
    For each: the library call alone (Batch.run) and end to end (Batch(...), run, results, the indexing, a device synchronisation).
    The two variants alternate round by round in one process; the masks are checked equal.

After --warmup untimed rounds, --rounds timed ones; a timed step lies between two device synchronisations.  One JSON line per
measurement: median, min, max over the rounds, in milliseconds.

    python scripts/device_results_bench.py
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

OPENCV = {"model": "OPENCV", "width": 1000, "height": 1000, "params": [1000.0, 1010.0, 500.0, 505.0, 0.04, -0.015, 8e-4, -6e-4]}


def report(name, times_ms, **extra):
    t = np.sort(np.array(times_ms))
    print(json.dumps(dict(name=name, median_ms=round(float(np.median(t)), 4), min_ms=round(float(t[0]), 4), max_ms=round(float(t[-1]), 4),
                          rounds=len(t), **extra)), flush=True)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--points", type=int, default=10000)
    ap.add_argument("--pairs", type=int, default=512)
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--streams", type=int, default=10, help="host threads inside the batch calls")
    args = ap.parse_args()

    import torch  # (first: the library then shares torch's HIP runtime and knows the tensors' memory)

    import poselib_amd as P
    from poselib_amd import _lib as L
    from poselib_amd import api, synth

    assert torch.cuda.is_available(), "no GPU: nothing is measured"
    torch.cuda.set_device(0)
    P.set_device(0)
    sync = torch.cuda.synchronize

    def timed(fn):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        return (time.perf_counter() - t0) * 1e3

    # ---------------------------------------------------------------- (a) undistortion
    V, N = args.views, args.points
    rng = np.random.default_rng(1)
    pix = rng.uniform(0.0, 1000.0, (V, N, 2))
    dist = np.stack([synth.opencv_distort_pixels(pix[v], OPENCV["params"]) for v in range(V)]).astype(np.float32)
    t = torch.from_numpy(dist).cuda()
    out = torch.empty((V, N, 2), dtype=torch.float64, device="cuda")
    cam = api._as_camera(OPENCV)._c()
    items = (L.UndistortItemDev * V)()
    keep = []
    for v in range(V):
        sd, n, owner = api._device_points(t[v], 2)
        od, o = api._device_points_out(out[v], n)
        items[v].camera, items[v].points2D, items[v].n, items[v].out = C.pointer(cam), sd, n, od
        keep.append((owner, o))
    lib = L.lib()

    def dev_call():
        L.check(lib.pl_undistort_points_batch_dev(items, V))

    def python_call():
        P.undistort_points_batch([(OPENCV, t[v], out[v]) for v in range(V)])

    trip = [None] * V

    def round_trip():
        for v in range(V):
            host = t[v].cpu().double().numpy()
            trip[v] = torch.from_numpy(P.undistort_points(OPENCV, host)).cuda()

    variants = {"undistort dev": dev_call, "undistort python": python_call, "undistort round trip": round_trip}
    times = {k: [] for k in variants}
    for r in range(args.warmup + args.rounds):
        for k, fn in variants.items():
            ms = timed(fn)
            if r >= args.warmup:
                times[k].append(ms)
    same = all((out[v].cpu().numpy().view(np.uint64) == trip[v].cpu().numpy().view(np.uint64)).all() for v in range(V))
    assert same, "device-to-device undistortion differs from the host call"
    med = {k: report(k, v, views=V, points=N) for k, v in times.items()}
    print(json.dumps(dict(name="undistort speed-up", dev_over_round_trip=round(med["undistort round trip"] / med["undistort dev"], 2),
                          points_per_s_dev=round(V * N / (med["undistort dev"] * 1e-3)), bit_equal=same)), flush=True)

    # ---------------------------------------------------------------- (b) masks
    B, R = args.pairs, args.rows
    host = np.zeros((B, R, 5), dtype=np.float32)
    for i in range(B):
        h = synth.homography_scene(R, 0.3, 1000 + i)
        host[i, :, :2], host[i, :, 2:4] = h["x1"], h["x2"]
        host[i, :, 4] = h["inlier_gt"] + 0.35 * rng.standard_normal(R)
    m = torch.from_numpy(host).cuda()
    mask = torch.zeros((B, R), dtype=torch.bool, device="cuda")
    opts = [{"ransac": {"seed": i}} for i in range(B)]
    picked = {}

    def run(device_masks):
        extra = (lambda i: {"inliers_out": mask[i]}) if device_masks else (lambda i: {})
        t0 = time.perf_counter()
        b = P.Batch([("hom", m[i, :, :2], m[i, :, 2:4], dict(opts[i], scores=m[i, :, 4], min_score=0.25, **extra(i))) for i in range(B)])
        sync()
        t1 = time.perf_counter()
        b.run(args.streams)
        t2 = time.perf_counter()
        res = b.results()
        if device_masks:
            sel = [m[i][mask[i]] for i in range(B)]
        else:
            sel = [m[i][torch.tensor(res[i][1]["inliers"], device="cuda")] for i in range(B)]
        sync()
        t3 = time.perf_counter()
        picked[device_masks] = (res, sel)
        return (t2 - t1) * 1e3, (t3 - t0) * 1e3

    call = {True: [], False: []}
    whole = {True: [], False: []}
    for r in range(args.warmup + args.rounds):
        for dm in ((True, False) if r % 2 == 0 else (False, True)):
            sync()
            c, w = run(dm)
            if r >= args.warmup:
                call[dm].append(c)
                whole[dm].append(w)
    (res_d, sel_d), (res_h, sel_h) = picked[True], picked[False]
    equal = all(torch.equal(a, b) for a, b in zip(sel_d, sel_h)) and all(
        np.ascontiguousarray(a[0]).tobytes() == np.ascontiguousarray(b[0]).tobytes() and a[1]["num_inliers"] == b[1]["num_inliers"]
        for a, b in zip(res_d, res_h))
    assert equal, "device masks differ from host masks"
    md = report("masks: library call, device masks", call[True], pairs=B, rows=R)
    mh = report("masks: library call, host masks", call[False], pairs=B, rows=R)
    wd = report("masks: end to end, device masks", whole[True], pairs=B, rows=R)
    wh = report("masks: end to end, host masks", whole[False], pairs=B, rows=R)
    print(json.dumps(dict(name="masks ratio", call_device_over_host=round(md / mh, 4), end_to_end_device_over_host=round(wd / wh, 4),
                          equal=equal, report=P.last_batch_report())), flush=True)


if __name__ == "__main__":
    main()
