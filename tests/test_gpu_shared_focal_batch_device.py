"""Batches of shared-focal pairs from device memory (-m gpu): every item of estimate_shared_focal_relative_pose_batch equals its
single device call and the host batch on the same values, bit for bit - pose, focal length, mask in the caller's numbering, n_used
and the stats - whatever its group, whatever runs next to it.  The grouped about-a-centre reduction in front of the groups is held
on its own against the plain Python loop."""
import ctypes as C
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from device_arrays import Allocation, DeviceArray, column_view, on_gpu, row_view
from device_results import download
from poselib_amd import _lib as L
from poselib_amd import synth
from test_gpu_uncalibrated_device_points import REDUCTION_SIZES, VIEWS, assert_same, loop_about, numpy_about, pixels, widened

pytestmark = pytest.mark.gpu

FILL = 0xAB
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def options(seed, **top):
    ransac = {"max_iterations": 1000, "min_iterations": 100, "seed": seed}
    ransac.update(top.pop("ransac", {}))
    return dict(top, max_error=2.0, ransac=ransac)


def pair_scene(n, ratio, seed):
    """(x1, x2, pp) of a synth scene with its own principal point; fewer than 40 rows: inliers only"""
    pp = (480.0 + 7.25 * (seed % 9), 510.0 - 3.5 * (seed % 5))
    d = synth.relative_pose_scene(max(n, 40), ratio, 9100 + seed, pp=pp)
    keep = np.arange(n) if n >= 40 else np.flatnonzero(d["inlier_gt"])[:n]
    return np.ascontiguousarray(d["x1"][keep]), np.ascontiguousarray(d["x2"][keep]), list(pp), d


def confidences(d, keep_n, seed, pad=0):
    """a matcher's confidences for the first keep_n rows (fp32, sixteenths: ties), NaN on the last `pad` rows"""
    rng = np.random.default_rng(700 + seed)
    gt = np.asarray(d["inlier_gt"], dtype=np.float64)[:keep_n]
    s = np.round((gt + 0.45 * rng.standard_normal(keep_n)).astype(np.float32) * 16) / np.float32(16)
    if pad:
        s[keep_n - pad:] = np.nan
    return s


def single(gpu, a, b, pp, opt, **kw):
    return gpu.estimate_shared_focal_relative_pose(a, b, pp, opt, kw.pop("initial_pair", None), **kw)


def batch_opt(opt, **extra):
    return dict(opt, **{k: v for k, v in extra.items() if v is not None})


# ------------------------------------------------------------------------------------------ 1. the grouped reduction alone
def test_the_grouped_reduction_carries_the_index_order_sums_bits(gpu):
    """members of 1 .. 513 rows (kStatsChunk is 256) in the five layouts, every member about a centre of its own, one call"""
    pairs, centres, want, tree = [], [], [], []
    for k, n in enumerate(REDUCTION_SIZES):
        x1, x2, c = pixels(n, 40 + n)
        for j, (name, (up, dtype)) in enumerate(sorted(VIEWS.items())):
            centre = (c[0] + 3.125 * k - 0.5 * j, c[1] - 11.0625 * j + k)
            w1, w2 = widened(x1, dtype), widened(x2, dtype)
            pairs.append((up(x1), up(x2)))
            centres.append(centre)
            want.append(repr(loop_about(w1, w2, centre)))
            tree.append(repr(numpy_about(w1, w2, centre)))
    got = [repr(s) for s in gpu.point_stats_about_group_dev(pairs, centres)]
    print("members", len(pairs), "whose numpy.sum differs from the loop:", sum(t != w for t, w in zip(tree, want)))
    assert any(t != w for t, w in zip(tree, want)), "the inputs would not show a sum in another order"
    assert got == want
    # ... and each equals the single launch about the same centre
    for (a, b), centre, w in list(zip(pairs, centres, want))[::7]:
        assert repr(gpu.point_stats_about_dev(a, b, centre)["scale"]) == w


# ------------------------------------------------------------------------------------------ 2. members
SIZES = (10, 11, 40, 255, 256, 257, 400, 640, 40, 256, 640, 255, 400, 257, 11)
RATIOS = (0.1, 0.3, 0.4)
_MEMBERS = {}


def members(gpu):
    """15 pairs in mixed layouts - views of ONE padded (pairs, 640, 5) fp32 tensor, fp64 contiguous, column and row views - with
    the results of the single device call and of the host batch on the widened values (computed once)"""
    if not _MEMBERS:
        scenes = [pair_scene(n, RATIOS[k % 3], k) for k, n in enumerate(SIZES)]
        padded = np.full((len(SIZES), 640, 5), np.nan, dtype=np.float32)
        for k, (x1, x2, pp, d) in enumerate(scenes):
            padded[k, :len(x1), :2], padded[k, :len(x1), 2:4] = x1, x2
        tensor = DeviceArray.upload(padded)
        pairs, host = [], []
        for k, (x1, x2, pp, d) in enumerate(scenes):
            n, opt, layout = len(x1), options(3 + k), k % 4
            if layout == 0:
                a, b, dtype = tensor[k, :n, :2], tensor[k, :n, 2:4], np.float32
            elif layout == 1:
                a, b, dtype = on_gpu(x1), on_gpu(x2), np.float64
            elif layout == 2:
                a, b, dtype = column_view(x1, np.float32), column_view(x2, np.float32), np.float32
            else:
                a, b, dtype = row_view(x1, np.float64), on_gpu(x2), np.float64
            pairs.append((a, b, pp, opt))
            host.append(("shared_focal", widened(x1, dtype), widened(x2, dtype), pp, opt))
        _MEMBERS["pairs"] = pairs
        _MEMBERS["single"] = [single(gpu, a, b, pp, opt) for a, b, pp, opt in pairs]
        _MEMBERS["host"] = gpu.estimate_batch(host)
    return _MEMBERS


@pytest.mark.parametrize("max_in_flight", [1, 4])
def test_every_item_equals_its_single_device_call_and_the_host_batch(gpu, max_in_flight):
    m = members(gpu)
    got = gpu.estimate_shared_focal_relative_pose_batch(m["pairs"], max_in_flight)
    report = gpu.last_batch_report()
    for k, n in enumerate(SIZES):
        print(k, n, "host inliers", m["host"][k][1]["num_inliers"], "iterations", m["host"][k][1]["iterations"])
        assert_same(got[k], m["single"][k], (k, n, "single device call"))
        assert_same(got[k], m["host"][k], (k, n, "host batch"))
        assert got[k][1]["n_used"] == n and len(got[k][1]["inliers"]) == n
        if n >= 40:  # (otherwise the test would pass on runs that never reach the final bundle)
            assert m["host"][k][1]["num_inliers"] > 6, (k, n)
    assert report == {"items": len(SIZES), "grouped": 0, "focal_grouped": len(SIZES), "solo": 0, "fallback": 0}


# ------------------------------------------------------------------------------------------ 3. what a group does not take
def test_items_a_group_does_not_take_run_alone_next_to_members(gpu):
    x1, x2, pp, d = pair_scene(300, 0.3, 31)
    warm = gpu.ImagePair(gpu.CameraPose(d["q_gt"], d["t_gt"]), gpu.Camera("SIMPLE_PINHOLE", [1100.0, pp[0], pp[1]]))
    few = np.full(300, -1.0)
    few[np.arange(8) * 17 + 5] = 1.0 + np.arange(8)
    a, b = on_gpu(x1, np.float32), column_view(x2, np.float64)
    cases = []  # (a, b, opt, keyword arguments of the single call, a member?)
    for n in (0, 5, 9):
        cases.append((on_gpu(x1[:n]), on_gpu(x2[:n]), options(n), {}, False))
    cases.append((a, b, options(4), {"initial_pair": warm}, False))
    cases.append((on_gpu(x1[:12]), on_gpu(x2[:12]), options(5, ransac={"min_iterations": 4097}), {}, False))
    cases.append((a, b, options(6), {"scores": on_gpu(few), "min_score": 0.0}, False))
    for k, n in enumerate((40, 100, 300)):
        cases.insert(2 * k, (on_gpu(x1[:n]), row_view(x2[:n], np.float64), options(20 + k), {}, True))
    want = [single(gpu, a, b, pp, opt, **kw) for a, b, opt, kw, _ in cases]
    got = gpu.estimate_shared_focal_relative_pose_batch([(a, b, pp, batch_opt(opt, **kw)) for a, b, opt, kw, _ in cases], 4)
    report = gpu.last_batch_report()
    for k, (g, w) in enumerate(zip(got, want)):
        assert_same(g, w, k)
    solo = sum(not member for *_, member in cases)
    assert solo == 6 and report == {"items": 9, "grouped": 0, "focal_grouped": 3, "solo": 6, "fallback": 0}
    assert got[-1][1]["n_used"] == 8 and len(got[-1][1]["inliers"]) == 300


# ------------------------------------------------------------------------------------------ 4. scores
def test_scored_items_are_ranked_first_and_form_groups_on_the_rows_left(gpu):
    cases = []
    for k, n in enumerate((400, 257, 640, 100)):
        x1, x2, pp, d = pair_scene(n, 0.3, 50 + k)
        s = confidences(d, n, k, pad=n // 10)
        m = float(np.sort(s[~np.isnan(s)])[n // 3])  # a threshold that is itself a tied value
        block = np.full((n, 5), 7e30, dtype=np.float32)
        block[:, :2], block[:, 2:4], block[:, 4] = x1, x2, s
        t = DeviceArray.upload(block)
        opt = options(8 + k, ransac={"progressive_sampling": True}) if k == 1 else options(8 + k)
        cases.append((t[:, :2], t[:, 2:4], pp, opt, t[:, 4], m, s, widened(x1, np.float32), widened(x2, np.float32)))
    x1, x2, pp, d = pair_scene(256, 0.3, 60)  # ... and a plain item among them
    pairs = [(a, b, pp, batch_opt(opt, scores=ds, min_score=m)) for a, b, pp, opt, ds, m, *_ in cases] + [(on_gpu(x1), on_gpu(x2), pp, options(1))]
    batch = gpu.SharedFocalBatch(pairs)
    batch.run(4)
    got = batch.results()
    report = gpu.last_batch_report()
    for k, (a, b, pp, opt, ds, m, s, wa, wb) in enumerate(cases):
        order = gpu.score_order(s, m)
        assert 0.4 * len(s) < len(order) < 0.8 * len(s) and np.isnan(s).sum() >= len(s) // 10
        want = single(gpu, a, b, pp, opt, scores=ds, min_score=m)
        assert_same(got[k], want, (k, "scored single call"))
        assert got[k][1]["n_used"] == batch.n_used[k] == len(order)
        host = single(gpu, wa[order], wb[order], pp, opt)  # the rule in numpy, the host call on the ranked rows
        flags = np.zeros(len(s), dtype=bool)
        flags[order] = host[1]["inliers"]
        assert got[k][1]["inliers"] == flags.tolist(), (k, "the mask speaks of the caller's rows")
        assert host[1]["num_inliers"] > 0.4 * len(order)
    assert_same(got[4], single(gpu, pairs[4][0], pairs[4][1], pairs[4][2], pairs[4][3]), "plain")
    assert batch.n_used[4] == 256
    assert report == {"items": 5, "grouped": 0, "focal_grouped": 5, "solo": 0, "fallback": 0}


# ------------------------------------------------------------------------------------------ 5. masks in device memory
def test_masks_go_to_device_memory_next_to_host_masks(gpu):
    n = 333
    x1, x2, pp, d = pair_scene(n, 0.3, 70)
    s = confidences(d, n, 70, pad=30)
    a, b, ds = on_gpu(x1), row_view(x2, np.float64), on_gpu(s)
    rows = DeviceArray.upload(np.ones((3, n), dtype=np.bool_))                # a bool row between two others
    cols = DeviceArray.upload(np.full((n, 4), FILL, dtype=np.uint8))          # a byte column of a wider block
    cols2 = DeviceArray.upload(np.full((n, 4), FILL, dtype=np.uint8))
    short = DeviceArray.upload(np.full((5, 3), FILL, dtype=np.uint8))
    few = np.full(n, -1.0)
    few[[3, 40, 200]] = 1.0
    lost = DeviceArray.upload(np.full((n, 2), FILL, dtype=np.uint8))
    cases = [(a, b, options(2), {"inliers_out": rows[1]}),
             (a, b, options(3), {}),                                                         # a host mask
             (a, b, options(4), {"scores": ds, "min_score": 0.25, "inliers_out": cols[:, 2]}),  # dropped rows: zeros
             (a, b, options(5), {"scores": ds, "min_score": 0.25}),                           # scored, host mask
             (on_gpu(x1[:5]), on_gpu(x2[:5]), options(6), {"inliers_out": short[:, 1]}),      # too few rows: zeros
             (a, b, options(7), {"scores": on_gpu(few), "min_score": 0.0, "inliers_out": lost[:, 0]}),  # too few rows left
             (a, b, options(8, ransac={"progressive_sampling": True}), {"inliers_out": cols2[:, 0]})]
    want = [single(gpu, a, b, pp, opt, **{k: v for k, v in kw.items() if k != "inliers_out"}) for a, b, opt, kw in cases]
    got = gpu.estimate_shared_focal_relative_pose_batch([(a, b, pp, batch_opt(opt, **kw)) for a, b, opt, kw in cases], 4)
    for k, (g, w) in enumerate(zip(got, want)):
        on_device = "inliers_out" in cases[k][3]
        assert_same(g, w, k, mask=not on_device)
        if on_device:
            assert g[1]["inliers"] is cases[k][3]["inliers_out"]
    assert want[0][1]["num_inliers"] > 0.3 * n and want[2][1]["num_inliers"] > 0.3 * want[2][1]["n_used"]
    back = download(rows)
    assert back[1].tolist() == want[0][1]["inliers"] and back[0].all() and back[2].all()
    assert set(back.view(np.uint8)[1].tolist()) <= {0, 1}
    back = download(cols)
    assert back[:, 2].tolist() == [int(v) for v in want[2][1]["inliers"]], "scored: the caller's rows, zeros where rows were dropped"
    assert not back[np.isnan(s) | (s < 0.25), 2].any() and (np.delete(back, 2, axis=1) == FILL).all()
    back = download(short)
    assert not back[:, 1].any() and (np.delete(back, 1, axis=1) == FILL).all()
    back = download(lost)
    assert got[5][1]["n_used"] == 3 and not back[:, 0].any() and (back[:, 1] == FILL).all()
    back = download(cols2)
    assert back[:, 0].tolist() == [int(v) for v in want[6][1]["inliers"]] and (back[:, 1:] == FILL).all()


# ------------------------------------------------------------------------------------------ 6. a rejected item
class TwiceTheReach:
    """a contiguous (n, 2) fp64 device array described with rows 4 elements apart: its rows reach beyond the allocation"""

    def __init__(self, arr):
        self.arr = arr

    @property
    def __cuda_array_interface__(self):
        cai = dict(self.arr.__cuda_array_interface__)
        cai["strides"] = (32, 8)
        return cai


def test_a_rejected_item_fails_alone(gpu):
    n = 200
    x1, x2, pp, d = pair_scene(n, 0.3, 80)
    a, b = on_gpu(x1), on_gpu(x2)
    pinned = DeviceArray(x1, x1.ctypes.data, Allocation(x1.nbytes, "pinned"))  # host memory the runtime knows (allocated, never touched)
    untouched = [DeviceArray.upload(np.full((n, 2), FILL, dtype=np.uint8)) for _ in range(2)]
    pairs = [(a, b, pp, options(1)),
             (a, b, pp, options(2)),
             (pinned, b, pp, batch_opt(options(3), inliers_out=untouched[0][:, 0])),
             (a, b, pp, options(4)),
             (a, TwiceTheReach(on_gpu(x2)), pp, batch_opt(options(5), inliers_out=untouched[1][:, 1])),
             (a, b, pp, options(6))]
    batch = gpu.SharedFocalBatch(pairs)
    with pytest.raises(gpu.PoseLibAmdError) as err:
        batch.run(4)
    msg = str(err.value)
    print(msg)
    assert f"error {L.PL_ERR_INVALID}:" in msg and "item 2:" in msg and "host memory" in msg, msg
    assert [batch.items[k].status for k in range(6)] == [0, 0, L.PL_ERR_INVALID, 0, L.PL_ERR_INVALID, 0]
    for u in untouched:
        assert (download(u) == FILL).all(), "a refused item's mask destination was written"
    got = batch.results()
    for k in (0, 1, 3, 5):
        assert_same(got[k], single(gpu, a, b, pp, pairs[k][3]), k)


# ------------------------------------------------------------------------------------------ 7. the group's shape does not matter
def test_results_do_not_depend_on_groups_workers_or_concurrent_calls(gpu):
    """40 eligible pairs of 40 rows - more than one group of 32 holds"""
    pairs = []
    for k in range(40):
        x1, x2, pp, d = pair_scene(40, RATIOS[k % 3], 100 + k)
        pairs.append((on_gpu(x1, np.float32), on_gpu(x2), pp, options(k, ransac={"max_iterations": 300, "min_iterations": 50})))

    def run(max_in_flight, out=None):
        r = gpu.estimate_shared_focal_relative_pose_batch(pairs, max_in_flight)
        if out is not None:
            out.append(r)
        return r

    want = run(8)
    assert gpu.last_batch_report() == {"items": 40, "grouped": 0, "focal_grouped": 40, "solo": 0, "fallback": 0}
    for k in (0, 13, 39):
        assert_same(want[k], single(gpu, *pairs[k]), k)
    before = os.environ.get("POSELIB_AMD_FOCAL_GROUP")
    try:
        for group in ("1", "3", None):
            if group is None:
                os.environ.pop("POSELIB_AMD_FOCAL_GROUP", None)
            else:
                os.environ["POSELIB_AMD_FOCAL_GROUP"] = group  # (read per call)
            for max_in_flight in (1, 8):
                for k, g in enumerate(run(max_in_flight)):
                    assert_same(g, want[k], (group, max_in_flight, k))
    finally:
        if before is None:
            os.environ.pop("POSELIB_AMD_FOCAL_GROUP", None)
        else:
            os.environ["POSELIB_AMD_FOCAL_GROUP"] = before
    # two host threads calling at once
    outs = [[], []]
    threads = [threading.Thread(target=run, args=(4, outs[i])) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for out in outs:
        assert len(out) == 1
        for k, g in enumerate(out[0]):
            assert_same(g, want[k], ("two threads", k))


# ------------------------------------------------------------------------------------------ 8. torch tensors
def test_torch_tensors_in_a_process_that_imports_torch_first(gpu):
    """views of one (pairs, N, 5) CUDA tensor, scores = its column 4, the masks in one (pairs, N) bool tensor"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "shared_focal_batch_device_torch_child.py")], capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    if r.returncode == 0 and "torch sees no GPU" in r.stdout:
        pytest.skip("torch sees no GPU")
    assert r.returncode == 0 and "torch shared-focal batch child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ------------------------------------------------------------------------------------------ 9. the refusals that stay
def test_the_kind_numbered_batch_and_Batch_still_refuse_shared_focal(gpu):
    x1, x2, pp, d = pair_scene(100, 0.3, 90)
    a, b = on_gpu(x1), on_gpu(x2)
    with pytest.raises(ValueError, match="shared_focal"):
        gpu.Batch([("shared_focal", a, b, pp, options(1))])
    items = (L.BatchItemDev * 2)()
    keep = []
    for it, kind in zip(items, (4, 2)):
        o = L.RobustOptions()
        L.lib().pl_default_robust_options(C.byref(o), 1 if kind == 4 else kind)
        o.ransac.max_iterations, o.ransac.min_iterations = 200, 50
        model, st, inl = np.zeros(9), L.RansacStats(), np.zeros(100, dtype=np.uint8)
        cam = gpu.Camera("SIMPLE_PINHOLE", [1.0, pp[0], pp[1]])._c()
        it.kind, it.n = kind, 100
        it.a = L.DevicePoints(a.data_ptr, 2, L.PL_F64, 2)
        it.b = L.DevicePoints(b.data_ptr, 2, L.PL_F64, 2)
        it.opt, it.camera1 = C.pointer(o), C.pointer(cam) if kind == 4 else None
        it.model, it.inliers, it.stats = model.ctypes.data, inl.ctypes.data, C.pointer(st)
        keep.append((o, model, st, inl, cam))
    assert L.lib().pl_estimate_batch_dev(items, 2, 4) == L.PL_ERR_UNSUPPORTED
    msg = L.lib().pl_last_error().decode()
    assert "item 0:" in msg and "kind 4" in msg, msg
    assert [it.status for it in items] == [L.PL_ERR_UNSUPPORTED, L.PL_OK] and keep[1][2].iterations > 0  # (the neighbour ran)
