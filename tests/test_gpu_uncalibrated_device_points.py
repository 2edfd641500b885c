"""Shared-focal relative pose and 1D-radial absolute pose from device memory (-m gpu): estimate_shared_focal_relative_pose and
estimate_1D_radial_absolute_pose on GPU arrays - fp64, fp32, strided views; with a matcher's scores; with the inlier mask written to
device memory - return what the host entry points return on the same values, bit for bit: the pose, the focal length, the mask and
every field of the stats but the seconds.  The two index-order reductions the device forms read back (pl_debug_point_stats_about_dev)
are held on their own against a plain Python loop, and the 1D-radial form against the reference's recorded runs."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from device_arrays import DeviceArray, column_view, on_gpu, row_view
from device_results import download
from golden import make_golden_radial1d as GR
from poselib_amd import synth

pytestmark = pytest.mark.gpu

STAT_KEYS = ("n_used", "refinements", "iterations", "num_inliers", "inlier_ratio", "model_score", "hypotheses", "iterations_evaluated",
             "nan_hypotheses")
KINDS = ("sfocal", "radial")
SAMPLE = {"sfocal": 6, "radial": 5}
FILL = 0xAB
G = json.load(open(GR.PATH))

VIEWS = {"fp64": (lambda x: on_gpu(x), np.float64),
         "fp32": (lambda x: on_gpu(x, np.float32), np.float32),
         "columns fp64": (lambda x: column_view(x, np.float64), np.float64),
         "columns fp32": (lambda x: column_view(x, np.float32), np.float32),
         "rows fp64": (lambda x: row_view(x, np.float64), np.float64)}


def widened(x, dtype):
    """the values a device array of `dtype` holds, as the doubles the library reads"""
    return np.ascontiguousarray(x, dtype=dtype).astype(np.float64)


# ------------------------------------------------------------------------------------------ the reductions alone
def pixels(n, seed):
    """two sets of pixels of order 10^3 with many mantissa bits, and a centre"""
    rng = np.random.default_rng(seed)
    return rng.uniform(-200.0, 2200.0, (n, 2)) * (1 + 1e-3 * rng.standard_normal((n, 2))), rng.uniform(0.0, 2000.0, (n, 2)), (1013.25, 987.0625)


def loop_about(x1, x2, c):
    """normalization_about (robust.cc:377-386 with utils.cc's scale): correspondence after correspondence"""
    scale = 0.0
    for (ax, ay), (bx, by) in zip(x1.tolist(), x2.tolist()):
        a0, a1, b0, b1 = ax - c[0], ay - c[1], bx - c[0], by - c[1]
        scale += math.sqrt(a0 * a0 + a1 * a1)
        scale += math.sqrt(b0 * b0 + b1 * b1)
    return scale / (math.sqrt(2) * len(x1))


def loop_radial(x):
    """robust.cc:904-907: n / sum |x_k|, and the largest |coordinate| of the scaled block"""
    total = 0.0
    for px, py in x.tolist():
        total += math.sqrt(0.0 + px * px + py * py)
    scale = float(len(x)) / total
    return scale, max(abs(v * scale) for v in x.ravel().tolist())


def numpy_about(x1, x2, c):
    terms = np.stack([np.sqrt(((x1 - c) ** 2).sum(1)), np.sqrt(((x2 - c) ** 2).sum(1))], axis=1).ravel()
    return float(np.sum(terms) / (math.sqrt(2) * len(x1)))


def numpy_radial(x):
    return float(len(x)) / float(np.sum(np.sqrt(0.0 + x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1])))


REDUCTION_SIZES = (1, 5, 255, 256, 257, 513)


@pytest.mark.parametrize("n", REDUCTION_SIZES)
def test_the_two_reductions_carry_the_index_order_sums_bits(gpu, n):
    x1, x2, c = pixels(n, 40 + n)
    for name, (up, dtype) in VIEWS.items():
        w1, w2 = widened(x1, dtype), widened(x2, dtype)
        got = gpu.point_stats_about_dev(up(x1), up(x2), c)
        want = loop_about(w1, w2, c)
        print(n, name, "about", repr(got["scale"]), repr(want), "numpy.sum", repr(numpy_about(w1, w2, c)))
        assert repr(got["scale"]) == repr(want), (n, name, "about a centre")
        got = gpu.point_stats_about_dev(up(x1))
        scale, amax = loop_radial(w1)
        print(n, name, "radial", repr(got["scale"]), repr(scale), "numpy.sum", repr(numpy_radial(w1)), "absmax", repr(got["absmax"]), repr(amax))
        assert (repr(got["scale"]), repr(got["absmax"])) == (repr(scale), repr(amax)), (n, name, "radial")


def test_these_inputs_would_show_a_tree_sum(gpu):
    """numpy.sum (pairwise, eight accumulators) gives another last bit than the index-order loop for some of the inputs above: a
    kernel that added in another order would not pass"""
    about, radial = [], []
    for n in REDUCTION_SIZES:
        x1, x2, c = pixels(n, 40 + n)
        for dtype in (np.float64, np.float32):
            w1, w2 = widened(x1, dtype), widened(x2, dtype)
            about.append(repr(numpy_about(w1, w2, c)) != repr(loop_about(w1, w2, c)))
            radial.append(repr(numpy_radial(w1)) != repr(loop_radial(w1)[0]))
    print("inputs whose numpy.sum differs from the loop: about a centre", sum(about), "radial", sum(radial), "of", len(about))
    assert any(about) and any(radial)


def test_the_radial_reduction_propagates_a_nan(gpu):
    x1, _, _ = pixels(300, 9)
    x1[123, 1] = np.nan
    got = gpu.point_stats_about_dev(on_gpu(x1))
    assert math.isnan(got["scale"]) and math.isnan(got["absmax"])
    x1, x2, c = pixels(300, 10)
    x2[7, 0] = np.nan
    assert math.isnan(gpu.point_stats_about_dev(on_gpu(x1), on_gpu(x2), c)["scale"])


# ------------------------------------------------------------------------------------------ the estimators
_SCENES = {}


def scene(kind, n, seed=0):
    """a synth scene at 30 % outliers with a matcher's confidences (fp32, sixteenths: ties; NaN on some rows) -> (a, b, pp, scores)"""
    key = (kind, n, seed)
    if key not in _SCENES:
        rng = np.random.default_rng(n + seed)
        if kind == "sfocal":
            d = synth.relative_pose_scene(max(n, 40), 0.3, 8800 + seed)
            a, b, pp = d["x1"], d["x2"], list(d["camera1"]["params"][1:3])
        else:
            d = synth.radial_1d_scene(max(n, 40), 0.3, 8900 + seed)
            a, b, pp = d["p2d"], d["p3d"], None
        keep = np.arange(len(a)) if n >= 40 else np.flatnonzero(d["inlier_gt"])[:n]  # (a minimal sample of inliers)
        gt = np.asarray(d["inlier_gt"], dtype=np.float64)[keep]
        s = (gt + 0.45 * rng.standard_normal(len(keep))).astype(np.float32)
        s = np.round(s * 16) / np.float32(16)
        s[::19] = np.nan
        _SCENES[key] = (np.ascontiguousarray(a[keep]), np.ascontiguousarray(b[keep]), pp, s, d)
    return _SCENES[key]


def options(seed, **top):
    ransac = {"max_iterations": 1000, "min_iterations": 100, "seed": seed}
    ransac.update(top.pop("ransac", {}))
    return dict(top, max_error=2.0, ransac=ransac)


def call(gpu, kind, a, b, pp, opt, initial=None, **kw):
    if kind == "sfocal":
        return gpu.estimate_shared_focal_relative_pose(a, b, pp, opt, initial, **kw)
    return gpu.estimate_1D_radial_absolute_pose(a, b, opt, initial, **kw)


def model_bits(m):
    if hasattr(m, "camera1"):
        return np.r_[m.pose.q, m.pose.t, m.camera1.params, m.camera2.params].view(np.uint64).tolist()
    return np.r_[m.q, m.t].view(np.uint64).tolist()  # (bit patterns: NaN equals NaN)


def assert_same(got, want, what, mask=True):
    (gm, gi), (wm, wi) = got, want
    for k in STAT_KEYS:
        assert gi[k] == wi[k] or (gi[k] != gi[k] and wi[k] != wi[k]), (what, k, gi[k], wi[k])
    assert repr(gi["model_score"]) == repr(wi["model_score"]), what
    assert model_bits(gm) == model_bits(wm), what
    if mask:
        assert gi["inliers"] == wi["inliers"], what


def warm_start(gpu, kind, d, pp):
    if kind == "sfocal":
        f = d["camera1"]["params"][0]
        return gpu.ImagePair(gpu.CameraPose(d["q_gt"], d["t_gt"]), gpu.Camera("SIMPLE_PINHOLE", [1.1 * f, pp[0], pp[1]]))
    rs = np.random.RandomState(3)
    q = d["q_gt"] + 0.01 * rs.randn(4)
    return gpu.CameraPose(q / np.linalg.norm(q), np.r_[d["t_gt"][:2], 0.0])


@pytest.mark.parametrize("view", sorted(VIEWS))
@pytest.mark.parametrize("n", [0, 257, 1000])  # (0: the minimal sample of the kind)
@pytest.mark.parametrize("kind", KINDS)
def test_device_points_equal_the_host_entry_point(gpu, kind, n, view):
    n = n or SAMPLE[kind]
    a, b, pp, s, d = scene(kind, n)
    up, dtype = VIEWS[view]
    wa, wb = widened(a, dtype), widened(b, dtype)
    da, db = up(a), up(b)
    opt = options(3 + n % 7)
    want = call(gpu, kind, wa, wb, pp, opt)
    got = call(gpu, kind, da, db, pp, opt)
    assert_same(got, want, (kind, n, view))
    assert got[1]["n_used"] == n and len(got[1]["inliers"]) == n
    if n >= 257:
        assert want[1]["num_inliers"] > 0.4 * n, (kind, n, "the scene is solved")
    if view in ("fp64", "columns fp32"):  # once warm, once with PROSAC
        init = warm_start(gpu, kind, d, pp)
        assert_same(call(gpu, kind, da, db, pp, opt, init), call(gpu, kind, wa, wb, pp, opt, init), (kind, n, view, "warm start"))
        prosac = options(11, ransac={"progressive_sampling": True})
        assert_same(call(gpu, kind, da, db, pp, prosac), call(gpu, kind, wa, wb, pp, prosac), (kind, n, view, "PROSAC"))


@pytest.mark.parametrize("kind", KINDS)
def test_fewer_rows_than_a_sample(gpu, kind):
    a, b, pp, s, d = scene(kind, 300)
    for n in (0, 1, SAMPLE[kind] - 1):
        opt = options(n)
        start = warm_start(gpu, kind, d, pp)
        want = call(gpu, kind, widened(a[:n], np.float32), b[:n], pp, opt, start)
        got = call(gpu, kind, on_gpu(a[:n].astype(np.float32)), column_view(b[:n], np.float64), pp, opt, start)
        assert_same(got, want, (kind, n))
        assert got[1]["iterations"] == 0


# ------------------------------------------------------------------------------------------ scores
@pytest.mark.parametrize("kind", KINDS)
def test_scored_equals_the_host_call_on_the_ranked_rows(gpu, kind):
    n = 400
    a, b, pp, s, d = scene(kind, n, 1)
    m = float(np.sort(s[~np.isnan(s)])[n // 3])  # a threshold that is itself a tied value
    order = gpu.score_order(s, m)
    assert 0.5 * n < len(order) < 0.8 * n and np.isnan(s).sum() > 10 and (s == np.float32(m)).sum() > 1
    assert len(set(s[order].tolist())) < len(order) // 4, "ties"
    da, db = column_view(a, np.float32), on_gpu(b)
    wa = widened(a, np.float32)
    block = np.full((n, 3), 7e30, dtype=np.float32)
    block[:, 2] = s
    for ds, opt in ((on_gpu(s), options(5)), (DeviceArray.upload(block)[:, 2], options(6, ransac={"progressive_sampling": True}))):
        want = call(gpu, kind, wa[order], b[order], pp, opt)
        got = call(gpu, kind, da, db, pp, opt, scores=ds, min_score=m)
        assert_same(got, want, (kind, "scored"), mask=False)
        assert got[1]["n_used"] == len(order)
        flags = np.zeros(n, dtype=bool)
        flags[order] = want[1]["inliers"]
        assert got[1]["inliers"] == flags.tolist()
        assert want[1]["num_inliers"] > 0.4 * len(order)
        # ... and the binding's rule for scores in host memory
        assert_same(call(gpu, kind, wa, b, pp, opt, scores=s, min_score=m), got, (kind, "scores on the host"))
    # too few rows survive
    for left in (0, 3, SAMPLE[kind] - 1):
        few = np.full(n, -1.0)
        few[np.arange(left) * 17 + 5] = 1.0 + np.arange(left)
        opt = options(7)
        order = gpu.score_order(few, 0.0)
        assert len(order) == left
        want = call(gpu, kind, wa[order], b[order], pp, opt)
        got = call(gpu, kind, da, db, pp, opt, scores=on_gpu(few), min_score=0.0)
        assert_same(got, want, (kind, left, "rows left"), mask=False)
        assert got[1]["n_used"] == left and not any(got[1]["inliers"]) and len(got[1]["inliers"]) == n


# ------------------------------------------------------------------------------------------ the mask in device memory
def destinations(n):
    """row 1 of a (3, n) block of bool-sized bytes and column 2 of an (n, 4) uint8 block, every byte 0xAB"""
    rows = DeviceArray.upload(np.full((3, n), FILL, dtype=np.uint8))
    cols = DeviceArray.upload(np.full((n, 4), FILL, dtype=np.uint8))
    return (rows, rows[1], lambda back: back[1], lambda back: np.delete(back, 1, axis=0)), \
           (cols, cols[:, 2], lambda back: back[:, 2], lambda back: np.delete(back, 2, axis=1))


@pytest.mark.parametrize("kind", KINDS)
def test_the_mask_goes_to_device_memory(gpu, kind):
    n = 333
    a, b, pp, s, d = scene(kind, n, 2)
    da, db = on_gpu(a), row_view(b, np.float64)
    ds = on_gpu(s)
    for scored in (False, True):
        kw = dict(scores=ds, min_score=0.25) if scored else {}
        opt = options(8 + scored)
        want = call(gpu, kind, da, db, pp, opt, **kw)
        assert want[1]["num_inliers"] > 0.3 * want[1]["n_used"]
        for buf, dst, flags, others in destinations(n):
            got = call(gpu, kind, da, db, pp, opt, inliers_out=dst, **kw)
            assert got[1]["inliers"] is dst
            assert_same(got, want, (kind, scored), mask=False)
            back = download(buf)
            assert flags(back).tolist() == [int(v) for v in want[1]["inliers"]], (kind, scored)
            assert (others(back) == FILL).all(), (kind, scored, "a neighbouring byte was written")
    # where the host form writes nothing, every byte is 0: too few rows left, and (1D radial) too few rows given
    few = np.full(n, -1.0)
    few[[3, 40, 200]] = 1.0
    for buf, dst, flags, others in destinations(n):
        got = call(gpu, kind, da, db, pp, options(1), scores=on_gpu(few), min_score=0.0, inliers_out=dst)
        back = download(buf)
        assert got[1]["n_used"] == 3 and got[1]["num_inliers"] == 0
        assert not flags(back).any() and (others(back) == FILL).all()
    if kind == "radial":
        for buf, dst, flags, others in destinations(4):
            got = call(gpu, kind, on_gpu(a[:4]), on_gpu(b[:4]), pp, options(1), inliers_out=dst)
            back = download(buf)
            assert got[1]["iterations"] == 0 and not flags(back).any() and (others(back) == FILL).all()


def test_torch_tensors_in_a_process_that_imports_torch_first(gpu):
    """a torch.bool row of a (3, N) tensor and a uint8 column of a wider one, float32 CUDA tensors of matches and scores"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "uncalibrated_device_torch_child.py")], capture_output=True, text=True,
                       timeout=300, cwd=root)
    if r.returncode == 0 and "torch sees no GPU" in r.stdout:
        pytest.skip("torch sees no GPU")
    assert r.returncode == 0 and "torch uncalibrated child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ------------------------------------------------------------------------------------------ against the reference's recorded runs
def api_options(opt):
    o = {k: (dict(v) if isinstance(v, dict) else v) for k, v in opt.items()}
    o.get("ransac", {}).pop("score_initial_model", None)  # (set by passing an initial pose)
    return o


@pytest.mark.parametrize("name", [c[0] for c in GR.EST_CASES])
def test_radial_from_device_memory_takes_the_references_decisions(gpu, name):
    """every recorded case of golden_radial1d_v1.json from device arrays, the refinements' sums in the reference's order
    (pl_set_lm_mode(1)): iterations, refinements, num_inliers, model_score, mask and pose of the reference's run, bit for bit"""
    case = [c for c in GR.EST_CASES if c[0] == name][0]
    rec = G["estimates"][name]
    d, opt, initial = GR.est_inputs(case, rec["data_seed"])
    assert GR.digest([d["p2d"], d["p3d"]]) == rec["input_sha256"], "the inputs changed: regenerate the fixture"
    start = [0.5, 0.5, -0.5, 0.5, 0.25, -2.0, 3.0]
    init = None if initial is None else gpu.CameraPose(initial[:4], initial[4:])
    if rec["n"] < 5:
        init = gpu.CameraPose(start[:4], start[4:])
    before = gpu.set_lm_mode(1)
    try:
        pose, info = gpu.estimate_1D_radial_absolute_pose(on_gpu(d["p2d"]), column_view(d["p3d"], np.float64), api_options(opt), init)
    finally:
        gpu.set_lm_mode(before)
    n = rec["n"]
    mask = np.unpackbits(np.frombuffer(bytes.fromhex(rec["mask_hex"]), dtype=np.uint8))[:n].astype(bool)
    assert (info["iterations"], info["refinements"], info["num_inliers"]) == (rec["iterations"], rec["refinements"], rec["num_inliers"])
    assert (np.array(info["inliers"], dtype=bool) == mask).all()
    if n < 5:  # (robust.cc:892-895: nothing runs)
        assert np.r_[pose.q, pose.t].tolist() == start and info["model_score"] == 0.0
        return
    assert repr(info["model_score"]) == rec["model_score"]
    assert repr(info["inlier_ratio"]) == rec["inlier_ratio"]
    assert GR.reprs(np.r_[pose.q, pose.t]) == rec["model"]
    assert pose.t[2] == 0.0


# ------------------------------------------------------------------------------------------ degenerate inputs
@pytest.mark.parametrize("kind", KINDS)
def test_a_nan_pixel_and_identical_points(gpu, kind):
    n = 300
    a, b, pp, s, d = scene(kind, n, 3)
    opt = options(2, ransac={"max_iterations": 200})
    bad = a.copy()
    bad[77, 1] = np.nan
    want = call(gpu, kind, bad, b, pp, opt)
    got = call(gpu, kind, on_gpu(bad), column_view(b, np.float64), pp, opt)
    assert_same(got, want, (kind, "a NaN pixel"))
    same_a, same_b = np.repeat(a[:1], n, axis=0), np.repeat(b[:1], n, axis=0)
    want = call(gpu, kind, same_a, same_b, pp, opt)
    got = call(gpu, kind, row_view(same_a, np.float64), on_gpu(same_b), pp, opt)
    assert_same(got, want, (kind, "identical points"))
