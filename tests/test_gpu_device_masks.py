"""Inlier masks written to device memory (pl_estimate_dev_masked / pl_estimate_batch_dev_masked; inliers_out= in Python): byte
i * stride of the destination is the host mask's flag of row i - for all n rows, dropped rows and items without a mask included -,
nothing else is touched, and model, stats, n_used and pl_last_batch_report are those of the call with a host mask."""
import os
import subprocess
import sys

import numpy as np
import pytest

from device_arrays import Allocation, DeviceArray, column_view, on_gpu, row_view
from device_results import download
from poselib_amd import _lib as L
from poselib_amd import synth

pytestmark = pytest.mark.gpu

STAT_KEYS = ("n_used", "refinements", "iterations", "num_inliers", "inlier_ratio", "model_score", "hypotheses", "iterations_evaluated",
             "nan_hypotheses")
KINDS = ("abs", "rel", "fund", "hom")
SAMPLE = {"abs": 3, "rel": 5, "fund": 7, "hom": 4}
FILL = 0xAA

_SCENES = {}


def scene(kind, n, seed=0):
    """a synth scene at 30 % outliers with a matcher's confidences: fp32, sixteenths (ties), NaN on some rows"""
    key = (kind, n, seed)
    if key not in _SCENES:
        make = {"abs": synth.absolute_pose_scene, "rel": synth.relative_pose_scene, "fund": synth.fundamental_scene,
                "hom": synth.homography_scene}[kind]
        d = make(n, 0.3, 700 + 10 * KINDS.index(kind) + seed)
        a, b = (d["p2d"], d["p3d"]) if kind == "abs" else (d["x1"], d["x2"])
        rng = np.random.default_rng(n + seed)
        s = (d["inlier_gt"] + 0.45 * rng.standard_normal(n)).astype(np.float32)
        s = np.round(s * 16) / np.float32(16)
        s[::19] = np.nan
        _SCENES[key] = (a, b, d, s)
    return _SCENES[key]


def options(seed, **top):
    ransac = {"max_iterations": 2000, "min_iterations": 100, "seed": seed}
    ransac.update(top.pop("ransac", {}))
    return dict(top, ransac=ransac)


def call(gpu, kind, a, b, d, opt, **kw):
    if kind == "abs":
        return gpu.estimate_absolute_pose(a, b, d["camera"], opt, None, **kw)
    if kind == "rel":
        return gpu.estimate_relative_pose(a, b, d["camera1"], d["camera2"], opt, None, **kw)
    return (gpu.estimate_fundamental if kind == "fund" else gpu.estimate_homography)(a, b, opt, None, **kw)


def problem(kind, a, b, d, opt):
    if kind == "abs":
        return ("abs", a, b, d["camera"], opt)
    if kind == "rel":
        return ("rel", a, b, d["camera1"], d["camera2"], opt)
    return (kind, a, b, opt)


def model_bytes(m):
    if hasattr(m, "pose"):
        return np.r_[m.pose.q, m.pose.t, m.camera.params].tobytes()
    if hasattr(m, "q"):
        return np.r_[m.q, m.t].tobytes()
    return np.ascontiguousarray(m, dtype=np.float64).tobytes()


def destination(n):
    """every second byte of a 2 n + 3 byte buffer of 0xAA: (the buffer, the n flags' view)"""
    buf = DeviceArray.upload(np.full(2 * n + 3, FILL, dtype=np.uint8))
    return buf, buf[0:2 * n:2]


def assert_mask(buf, n, want_mask, what):
    back = download(buf)
    assert back[0:2 * n:2].tolist() == [int(v) for v in want_mask], what
    assert (back[1:2 * n:2] == FILL).all() and (back[2 * n:] == FILL).all(), what  # the odd bytes and the tail


def assert_same(got, want, what):
    (gm, gi), (wm, wi) = got, want
    for k in STAT_KEYS:
        assert gi[k] == wi[k], (what, k, gi[k], wi[k])
    assert repr(gi["model_score"]) == repr(wi["model_score"]), what
    assert model_bytes(gm) == model_bytes(wm), what


UPLOADS = {"abs": (lambda x: on_gpu(x), lambda x: row_view(x, np.float64)),
           "rel": (lambda x: column_view(x, np.float32), lambda x: on_gpu(x, np.float32)),
           "fund": (lambda x: on_gpu(x), lambda x: column_view(x, np.float64)),
           "hom": (lambda x: on_gpu(x, np.float32), lambda x: column_view(x, np.float32))}


@pytest.mark.parametrize("kind", KINDS)
def test_the_four_kinds_with_and_without_scores(gpu, kind):
    n = 300 + 25 * KINDS.index(kind)
    a, b, d, s = scene(kind, n)
    da, db = UPLOADS[kind][0](a), UPLOADS[kind][1](b)
    opt = options(5)
    # without scores: the existing _dev call
    want = call(gpu, kind, da, db, d, opt)
    buf, dst = destination(n)
    got = call(gpu, kind, da, db, d, opt, inliers_out=dst)
    assert got[1]["inliers"] is dst
    assert_same(got, want, (kind, "plain"))
    assert_mask(buf, n, want[1]["inliers"], (kind, "plain"))
    assert want[1]["num_inliers"] > 0.3 * n, (kind, "the scene is solved")
    # with scores: fp32, a threshold that drops about a third of the rows (NaN rows among them) and is itself a tied value
    m = float(np.sort(s[~np.isnan(s)])[n // 3])
    kept = gpu.score_order(s, m)
    assert 0.55 * n < len(kept) < 0.8 * n and np.isnan(s).sum() > 10 and (s == np.float32(m)).sum() > 1
    ds = on_gpu(s)
    want = call(gpu, kind, da, db, d, opt, scores=ds, min_score=m)
    buf, dst = destination(n)
    got = call(gpu, kind, da, db, d, opt, scores=ds, min_score=m, inliers_out=dst)
    assert_same(got, want, (kind, "scored"))
    assert got[1]["n_used"] == len(kept)
    assert_mask(buf, n, want[1]["inliers"], (kind, "scored"))
    dropped = np.ones(n, dtype=bool)
    dropped[kept] = False
    assert not np.array(want[1]["inliers"])[dropped].any() and want[1]["num_inliers"] > 0.3 * len(kept)
    # PROSAC over the ranked rows, scores as a column of a wider block
    opt = options(6, ransac={"progressive_sampling": True})
    block = np.full((n, 3), 7e30, dtype=np.float32)
    block[:, 2] = s
    ds = DeviceArray.upload(block)[:, 2]
    want = call(gpu, kind, da, db, d, opt, scores=ds, min_score=0.25)
    buf, dst = destination(n)
    got = call(gpu, kind, da, db, d, opt, scores=ds, min_score=0.25, inliers_out=dst)
    assert_same(got, want, (kind, "prosac"))
    assert_mask(buf, n, want[1]["inliers"], (kind, "prosac"))


@pytest.mark.parametrize("kind", KINDS)
def test_fewer_rows_than_the_estimator_needs(gpu, kind):
    """n below the minimum, and scores that keep fewer: all n bytes are 0 where the host form writes no mask, and the host form's
    flags where it writes one (an absolute or relative pose of fewer rows than a sample scores its untouched model)"""
    a, b, d, s = scene(kind, 300)
    for n in (1, SAMPLE[kind] - 1):
        da, db = on_gpu(a[:n]), on_gpu(b[:n])
        want = call(gpu, kind, da, db, d, options(3))
        buf, dst = destination(n)
        got = call(gpu, kind, da, db, d, options(3), inliers_out=dst)
        assert_same(got, want, (kind, n))
        assert_mask(buf, n, want[1]["inliers"], (kind, n))
        assert want[1]["iterations"] == 0 and want[1]["refinements"] == 0
        if kind in ("fund", "hom"):
            assert not any(want[1]["inliers"])
    n = 40
    da, db, ds = on_gpu(a[:n]), on_gpu(b[:n]), on_gpu(np.arange(n, dtype=np.float32))
    for kept in (0, SAMPLE[kind] - 1):
        m = np.inf if kept == 0 else float(n - kept)
        want = call(gpu, kind, da, db, d, options(3), scores=ds, min_score=m)
        buf, dst = destination(n)
        got = call(gpu, kind, da, db, d, options(3), scores=ds, min_score=m, inliers_out=dst)
        assert_same(got, want, (kind, "kept", kept))
        assert got[1]["n_used"] == kept
        assert_mask(buf, n, want[1]["inliers"], (kind, "kept", kept))


def test_a_destination_the_library_cannot_write_is_refused_and_untouched(gpu):
    a, b, d, s = scene("hom", 300)
    da, db = on_gpu(a), on_gpu(b)
    flags = np.full(300, FILL, dtype=np.uint8)
    pinned = DeviceArray(flags, flags.ctypes.data, Allocation(flags.nbytes, "pinned"))  # (allocated, never touched)
    with pytest.raises(gpu.PoseLibAmdError) as e:
        gpu.estimate_homography(da, db, options(1), inliers_out=pinned)
    assert f"error {L.PL_ERR_INVALID}:" in str(e.value) and "device mask" in str(e.value) and "host memory" in str(e.value)
    short = DeviceArray.upload(np.full(299, FILL, dtype=np.uint8))
    with pytest.raises(gpu.PoseLibAmdError) as e:  # the extent: 300 flags are asked of an allocation of 299 bytes
        gpu.estimate_homography(da, db, options(1), inliers_out=DeviceArray(flags, flags.ctypes.data, short.allocation))
    assert "device mask" in str(e.value) and "beyond the allocation" in str(e.value)
    assert (download(short) == FILL).all()


def batch_specs():
    """12 items over the four kinds, n from 40 to 600: (kind, device a, device b, scene, options, device scores or None, min_score)"""
    specs = []

    def add(kind, n, seed, opt, scored=False, uploads=None):
        a, b, d, s = scene(kind, n, seed)
        ua, ub = uploads or UPLOADS[kind]
        specs.append((kind, ua(a), ub(b), d, opt, on_gpu(s) if scored else None, 0.25 if scored else None, n))

    add("abs", 600, 1, options(20))
    add("rel", 350, 2, options(21))
    add("fund", 300, 3, options(22), scored=True)                                   # scored
    add("hom", 400, 4, options(23, ransac={"progressive_sampling": True}), scored=True)  # scored, PROSAC over the ranked rows
    add("hom", 257, 5, options(24, ransac={"progressive_sampling": True}))          # PROSAC
    add("rel", 320, 6, options(25, tangent_sampson=True))                           # runs solo
    add("fund", SAMPLE["fund"] + 3, 7, options(26))                                 # sample size + 3: runs solo
    add("abs", 40, 8, options(27))
    add("hom", 64, 9, options(28), uploads=(lambda x: on_gpu(x), lambda x: on_gpu(x)))
    add("fund", 511, 10, options(29))
    add("rel", 100, 11, options(30))
    add("abs", 333, 12, options(31), scored=True)
    assert len(specs) == 12
    return specs


def batch_items(specs, masks):
    items = []
    for (kind, da, db, d, opt, ds, m, n), mask in zip(specs, masks):
        o = dict(opt)
        if ds is not None:
            o.update(scores=ds, min_score=m)
        if mask is not None:
            o["inliers_out"] = mask
        items.append(problem(kind, da, db, d, o))
    return items


def test_a_batch_of_twelve_items(gpu):
    specs = batch_specs()
    HOST_ITEM = 9  # masks[i].data == NULL: the item keeps its host mask
    want = gpu.estimate_batch(batch_items(specs, [None] * 12))  # pl_estimate_batch_dev_scored: host masks
    want_report = gpu.last_batch_report()
    assert want_report["items"] == 12 and want_report["solo"] == 2 and want_report["grouped"] == 10, want_report
    dests = [destination(spec[7]) for spec in specs]
    masks = [None if i == HOST_ITEM else dests[i][1] for i in range(12)]
    batch = gpu.Batch(batch_items(specs, masks))
    assert batch.masked and batch.scored and not batch.masks[HOST_ITEM].data
    batch.run()
    report = gpu.last_batch_report()
    got = batch.results()
    assert report == want_report, (report, want_report)
    for i, (g, w) in enumerate(zip(got, want)):
        assert_same(g, w, ("batch", i))
        n = specs[i][7]
        if i == HOST_ITEM:
            assert g[1]["inliers"] == w[1]["inliers"]
            assert (download(dests[i][0]) == FILL).all()
        else:
            assert g[1]["inliers"] is masks[i]
            assert_mask(dests[i][0], n, w[1]["inliers"], ("batch", i))
        if w[1]["n_used"] >= 100:
            assert w[1]["num_inliers"] > 0.25 * w[1]["n_used"], ("the scene is solved", i)
    # ... and with one bad destination: that item fails alone, its memory is not touched, the others are what they were
    BAD = 4
    flags = np.full(specs[BAD][7], FILL, dtype=np.uint8)
    pinned = DeviceArray(flags, flags.ctypes.data, Allocation(flags.nbytes, "pinned"))  # (allocated, never touched)
    dests = [destination(spec[7]) for spec in specs]
    masks = [None if i == HOST_ITEM else (pinned if i == BAD else dests[i][1]) for i in range(12)]
    batch = gpu.Batch(batch_items(specs, masks))
    with pytest.raises(gpu.PoseLibAmdError) as e:
        batch.run()
    assert f"error {L.PL_ERR_INVALID}:" in str(e.value) and f"item {BAD}:" in str(e.value) and "device mask" in str(e.value)
    assert [it.status for it in batch.items] == [L.PL_ERR_INVALID if i == BAD else L.PL_OK for i in range(12)]
    got = batch.results()
    for i, (g, w) in enumerate(zip(got, want)):
        if i == BAD:
            assert (download(dests[i][0]) == FILL).all()
            continue
        assert_same(g, w, ("batch with a bad item", i))
        if i != HOST_ITEM:
            assert_mask(dests[i][0], specs[i][7], w[1]["inliers"], ("batch with a bad item", i))


def test_the_masks_do_not_depend_on_the_prefilter(gpu):
    """the single calls of the four kinds again, in a fresh process with POSELIB_AMD_NO_PREFILTER=1 (every pair evaluated exactly)"""
    if os.environ.get("POSELIB_AMD_NO_PREFILTER"):
        return
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k",
                        "test_the_four_kinds_with_and_without_scores"], env=dict(os.environ, POSELIB_AMD_NO_PREFILTER="1"),
                       capture_output=True, text=True, timeout=300, cwd=root)
    assert r.returncode == 0 and "4 passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_torch_tensors_in_a_process_that_imports_torch_first(gpu):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "device_results_torch_child.py")], capture_output=True, text=True,
                       timeout=300, cwd=root)
    if r.returncode == 0 and "torch sees no GPU" in r.stdout:
        pytest.skip("torch sees no GPU")
    assert r.returncode == 0 and "torch device results child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
