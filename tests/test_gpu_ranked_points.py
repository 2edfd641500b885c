"""Device-resident matches with their confidences (scores= / pl_estimate_dev_scored / pl_estimate_batch_dev_scored) on the device:
a scored call is, bit for bit, the existing HOST call on the rows a[order], b[order] - order from the rule's numpy statement
(poselib_amd.score_order) -, with the mask back in the caller's numbering; a batch item equals its single call and the batch goes
where the host batch on the pre-sorted, compacted arrays goes."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
from device_arrays import Allocation, DeviceArray, column_view, on_gpu, row_view
from poselib_amd import _lib as L
from poselib_amd import score_order, synth

pytestmark = pytest.mark.gpu

STAT_KEYS = ("refinements", "iterations", "num_inliers", "inlier_ratio", "model_score", "hypotheses")
KINDS = ("abs", "rel", "fund", "hom")
SAMPLE = {"abs": 3, "rel": 5, "fund": 7, "hom": 4}
OPENCV = [1000.0, 1000.0, 500.0, 500.0, -0.08, 0.02, 0.001, -0.0005]
WARM_H = np.array([[1.0, 0.01, 3.0], [-0.01, 1.0, -2.0], [1e-5, -1e-5, 1.0]])

_SCENES = {}


def scene(kind, n, seed=0):
    key = (kind, n, seed)
    if key not in _SCENES:
        make = {"abs": synth.absolute_pose_scene, "rel": synth.relative_pose_scene, "fund": synth.fundamental_scene,
                "hom": synth.homography_scene}[kind]
        d = make(n, 0.4, 300 + 10 * KINDS.index(kind) + seed)
        a, b = (d["p2d"], d["p3d"]) if kind == "abs" else (d["x1"], d["x2"])
        rng = np.random.default_rng(n + seed)
        s = (d["inlier_gt"] + 0.4 * rng.standard_normal(n)).astype(np.float32)  # a confidence: higher on inliers, with ties of
        s = np.round(s * 16) / np.float32(16)                                   # its own (sixteenths) ...
        s[::23] = np.nan                                                        # ... and padding rows
        _SCENES[key] = (a, b, d, s)
    return _SCENES[key]


def options(seed, **top):
    ransac = {"max_iterations": 2000, "min_iterations": 100, "seed": seed}
    ransac.update(top.pop("ransac", {}))
    return dict(top, ransac=ransac)


def call(gpu, kind, a, b, d, opt, camera=None, initial=None, **kw):
    if kind == "abs":
        return gpu.estimate_absolute_pose(a, b, camera or d["camera"], opt, initial, **kw)
    if kind == "rel":
        return gpu.estimate_relative_pose(a, b, d["camera1"], d["camera2"], opt, initial, **kw)
    return (gpu.estimate_fundamental if kind == "fund" else gpu.estimate_homography)(a, b, opt, initial, **kw)


def model_bytes(m):
    if hasattr(m, "pose"):  # Image
        return np.r_[m.pose.q, m.pose.t, m.camera.params].tobytes()
    if hasattr(m, "q"):
        return np.r_[m.q, m.t].tobytes()
    return np.ascontiguousarray(m, dtype=np.float64).tobytes()


def assert_same(got, want, order, n, what, n_used=None):
    """got: a scored call over n rows; want: the host call on the rows `order` (n_used: another count than len(order) is expected)"""
    (gm, gi), (wm, wi) = got, want
    for k in STAT_KEYS:
        assert gi[k] == wi[k], (what, k, gi[k], wi[k])
    assert repr(gi["model_score"]) == repr(wi["model_score"]), what
    mask = np.zeros(n, dtype=bool)
    mask[order] = wi["inliers"]
    assert gi["inliers"] == mask.tolist(), what
    assert gi["n_used"] == (len(order) if n_used is None else n_used), (what, gi["n_used"], len(order))
    assert model_bytes(gm) == model_bytes(wm), what


# how the points (two sets) and the scores of an item lie in device memory: name -> (points upload, points are fp32, scores upload)
def scores_column(s, dtype):
    block = np.full((len(s), 5), 7e30, dtype=dtype)
    block[:, 4] = s
    return DeviceArray.upload(block)[:, 4]


FORMS = {
    "fp64": (lambda x: on_gpu(x), False, lambda s: on_gpu(s.astype(np.float64))),
    "fp32_columns": (lambda x: column_view(x, np.float32), True, lambda s: scores_column(s, np.float32)),
    "fp64_rows": (lambda x: row_view(x, np.float64), False, lambda s: scores_column(s, np.float64)),
    "fp32": (lambda x: on_gpu(x, np.float32), True, lambda s: on_gpu(s)),
}


def widened(x, f32):
    return x.astype(np.float32).astype(np.float64) if f32 else x


# ---------------------------------------------------------------- 5: the estimators
@pytest.mark.parametrize("prosac", [False, True], ids=["uniform", "prosac"])
@pytest.mark.parametrize("kind", KINDS)
def test_scored_device_call_equals_host_call_on_the_ranked_rows(gpu, kind, prosac):
    n = 300
    a, b, d, s = scene(kind, n)
    opt = options(5, ransac={"progressive_sampling": prosac})
    for i, form in enumerate(FORMS):
        upload, f32, upload_scores = FORMS[form]
        m = (None, 0.25, 0.5, 0.3)[i]  # -inf, a tied value (sixteenths), another, a value between scores
        order = score_order(s, m)
        assert SAMPLE[kind] + 4 < len(order) < n
        ha, hb = widened(a, f32), widened(b, f32)
        want = call(gpu, kind, ha[order], hb[order], d, opt)
        got = call(gpu, kind, upload(a), upload(b), d, opt, scores=upload_scores(s), min_score=m)
        assert_same(got, want, order, n, (kind, prosac, form))
        if i == 0:  # ... and the expectation does not rest on this library alone: the oracle on the sorted rows
            ref = {"abs": lambda: O.estimate_absolute_pose(ha[order], hb[order], d["camera"], opt),
                   "rel": lambda: O.estimate_relative_pose(ha[order], hb[order], d["camera1"], d["camera2"], opt),
                   "fund": lambda: O.estimate_fundamental(ha[order], hb[order], opt),
                   "hom": lambda: O.estimate_homography(ha[order], hb[order], opt)}[kind]()
            info = got[1]
            assert info["iterations"] == ref[2]["iterations"] and info["num_inliers"] == ref[2]["num_inliers"], (kind, prosac)
            mask = np.zeros(n, dtype=bool)
            mask[order] = ref[1]
            assert info["inliers"] == mask.tolist(), (kind, prosac)
            # not a degenerate scene: 60 % of the rows are true inliers; the planar scene's default threshold keeps about two
            # thirds of those (the oracle says the same), so "solved" is a clear majority of them, not all
            assert info["num_inliers"] > 0.3 * len(order), (kind, "the scene is solved")


@pytest.mark.parametrize("kind", KINDS)
def test_small_kept_counts_are_the_host_forms_at_that_n(gpu, kind):
    """all rows dropped, fewer than a sample, sample size + 3 and + 4 (the edges of a group, and where the host forms change)"""
    n = 120
    a, b, d, _ = scene(kind, n, seed=1)
    s = np.random.default_rng(3).permutation(n).astype(np.float64)  # distinct: min_score = n - k keeps exactly k rows
    da, db, ds = on_gpu(a), column_view(b, np.float64), on_gpu(s)
    k0 = SAMPLE[kind]
    for kept in (0, k0 - 1, k0, k0 + 3, k0 + 4):
        m = np.inf if kept == 0 else float(n - kept)
        order = score_order(s, m)
        assert len(order) == kept
        opt = options(9, ransac={"progressive_sampling": True})
        want = call(gpu, kind, a[order], b[order], d, opt)
        got = call(gpu, kind, da, db, d, opt, scores=ds, min_score=m)
        assert_same(got, want, order, n, (kind, kept))


def test_warm_start_and_opencv_camera(gpu):
    n = 300
    a, b, d, s = scene("hom", n, seed=2)
    order = score_order(s, 0.25)
    opt = options(11, ransac={"progressive_sampling": True})
    want = gpu.estimate_homography(a[order], b[order], opt, WARM_H)
    got = gpu.estimate_homography(on_gpu(a), on_gpu(b), opt, WARM_H, scores=scores_column(s, np.float32), min_score=0.25)
    assert_same(got, want, order, n, "warm start")
    a, b, d, s = scene("abs", n, seed=2)
    pix = synth.opencv_distort_pixels(a, OPENCV)
    cam = {"model": "OPENCV", "params": OPENCV}
    order = score_order(s)
    want = gpu.estimate_absolute_pose(pix[order], b[order], cam, opt)
    got = gpu.estimate_absolute_pose(column_view(pix, np.float64), on_gpu(b), cam, opt, scores=on_gpu(s))
    assert_same(got, want, order, n, "OPENCV")


def test_what_the_plain_call_refuses_the_scored_call_refuses(gpu):
    a, b, d, s = scene("abs", 300)
    with pytest.raises(gpu.PoseLibAmdError) as e:
        gpu.estimate_absolute_pose(on_gpu(a), on_gpu(b), d["camera"], options(1, estimate_focal_length=True), scores=on_gpu(s))
    assert f"error {L.PL_ERR_UNSUPPORTED}:" in str(e.value) and "estimate_focal_length" in str(e.value)
    pinned = DeviceArray(s, s.ctypes.data, Allocation(s.nbytes, "pinned"))  # (allocated, never touched)
    with pytest.raises(gpu.PoseLibAmdError) as e:
        gpu.estimate_absolute_pose(on_gpu(a), on_gpu(b), d["camera"], options(1), scores=pinned)
    assert f"error {L.PL_ERR_INVALID}:" in str(e.value) and "device scores" in str(e.value) and "host memory" in str(e.value)
    short, longer = on_gpu(s[:200]), np.zeros(300, dtype=np.float32)
    with pytest.raises(gpu.PoseLibAmdError) as e:  # the extent: 300 scores are asked of an allocation of 200
        gpu.rank_scores(DeviceArray(longer, longer.ctypes.data, short.allocation))
    assert "device scores" in str(e.value) and "beyond the allocation" in str(e.value)
    # tangent Sampson is served, as a solo item, like the plain call
    a, b, d, s = scene("rel", 300)
    order = score_order(s, 0.25)
    opt = options(3, tangent_sampson=True)
    want = call(gpu, "rel", a[order], b[order], d, opt)
    got = call(gpu, "rel", on_gpu(a), on_gpu(b), d, opt, scores=on_gpu(s), min_score=0.25)
    assert_same(got, want, order, 300, "tangent")


# ---------------------------------------------------------------- 6: the batch
def problem(kind, a, b, d, opt):
    if kind == "abs":
        return ("abs", a, b, d["camera"], opt)
    if kind == "rel":
        return ("rel", a, b, d["camera1"], d["camera2"], opt)
    return (kind, a, b, opt)


def test_a_batch_of_scored_and_plain_items(gpu):
    pairs, N = 6, 400
    # one padded (pairs, N, 5) fp32 block, as a matcher leaves it: x1, x2, confidence; the rows behind a pair's matches are padding
    block = np.zeros((pairs, N, 5), dtype=np.float32)
    valid = (400, 37, 250, 400, 11, 120)
    two_view = ("hom", "fund", "rel", "hom", "fund", "hom")
    for i in range(pairs):
        a, b, d, s = scene(two_view[i], N, seed=10 + i)
        block[i, :, :2], block[i, :, 2:4], block[i, :, 4] = a, b, s
        block[i, valid[i]:, 4] = np.nan if i % 2 else -1.0
    dev_block = DeviceArray.upload(block)
    wide = block.astype(np.float64)
    specs = []  # (kind, host a, host b, host scores or None, min_score, device a, device b, device scores, extras, options)
    for i in range(pairs):
        d = scene(two_view[i], N, seed=10 + i)[2]
        m = (0.0, None, 0.25, 0.5, 0.0, 0.3)[i]
        specs.append((two_view[i], wide[i, :, :2], wide[i, :, 2:4], block[i, :, 4], m, dev_block[i, :, :2], dev_block[i, :, 2:4],
                      dev_block[i, :, 4], d, options(40 + i, ransac={"progressive_sampling": i % 2 == 0})))
    # item 4: 11 valid rows, a threshold that keeps fewer than sample size + 4 of them -> solo
    assert len(score_order(block[4, :, 4], 0.0)) < SAMPLE["fund"] + 4
    # absolute pose, fp64, scored; a plain item; more than 16384 rows of which fewer are kept
    a, b, d, s = scene("abs", 300)
    specs.append(("abs", a, b, s, 0.25, on_gpu(a), row_view(b, np.float64), on_gpu(s.astype(np.float64)), d, options(50)))
    a, b, d, s = scene("hom", 300, seed=3)
    specs.append(("hom", a, b, None, None, on_gpu(a), on_gpu(b), None, d, options(51)))
    a, b, d, s = scene("hom", 17000)
    specs.append(("hom", a, b, s, 0.75, column_view(a, np.float64), on_gpu(b), on_gpu(s), d, options(52, ransac={"progressive_sampling": True})))
    assert SAMPLE["hom"] + 4 <= len(score_order(s, 0.75)) <= 16384

    host_items, dev_items, orders = [], [], []
    for kind, ha, hb, hs, m, da, db, ds, d, opt in specs:
        order = np.arange(len(ha)) if hs is None else score_order(hs, m)
        orders.append(order)
        host_items.append(problem(kind, ha[order], hb[order], d, opt))
        dev_items.append(problem(kind, da, db, d, opt if hs is None else dict(opt, scores=ds, min_score=m)))
    want = gpu.estimate_batch(host_items)
    want_report = gpu.last_batch_report()
    got = gpu.estimate_batch(dev_items)
    report = gpu.last_batch_report()
    for i, (spec, g, w) in enumerate(zip(specs, got, want)):
        assert_same(g, w, orders[i], len(spec[1]), ("batch", i))
    assert report == want_report, (report, want_report)
    assert report["items"] == len(specs) and report["solo"] == 1 and report["grouped"] == len(specs) - 1
    # every item equals its single scored call
    for i, (kind, ha, hb, hs, m, da, db, ds, d, opt) in enumerate(specs):
        single = call(gpu, kind, da, db, d, opt) if hs is None else call(gpu, kind, da, db, d, opt, scores=ds, min_score=m)
        assert_same(got[i], single, np.arange(len(ha)), len(ha), ("single", i), n_used=len(orders[i]))
        assert single[1]["n_used"] == len(orders[i])


def test_bad_scores_fail_their_own_item_only(gpu):
    items, hosts = [], []
    for i in range(4):
        a, b, d, s = scene("hom", 300, seed=20 + i)
        order = score_order(s, 0.25)
        hosts.append(("hom", a[order], b[order], options(i)))
        items.append(("hom", on_gpu(a), on_gpu(b), dict(options(i), scores=on_gpu(s), min_score=0.25)))
    want = gpu.estimate_batch(hosts)
    s = scene("hom", 300, seed=22)[3]
    pinned = DeviceArray(s, s.ctypes.data, Allocation(s.nbytes, "pinned"))  # (allocated, never touched)
    items[2] = items[2][:3] + (dict(items[2][3], scores=pinned),)
    batch = gpu.Batch(items)
    with pytest.raises(gpu.PoseLibAmdError) as e:
        batch.run()
    assert f"error {L.PL_ERR_INVALID}:" in str(e.value) and "item 2:" in str(e.value) and "device scores" in str(e.value)
    assert [it.status for it in batch.items] == [L.PL_OK, L.PL_OK, L.PL_ERR_INVALID, L.PL_OK]
    got = batch.results()
    for i in (0, 1, 3):
        order = score_order(scene("hom", 300, seed=20 + i)[3], 0.25)
        assert_same(got[i], want[i], order, 300, i)


# ---------------------------------------------------------------- 7: torch
def test_the_scores_column_of_one_torch_tensor_in_a_process_that_imports_torch_first(gpu):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "ranked_points_torch_child.py")], capture_output=True, text=True,
                       timeout=300, cwd=root)
    if r.returncode == 0 and "torch sees no GPU" in r.stdout:
        pytest.skip("torch sees no GPU")
    assert r.returncode == 0 and "torch ranked child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
