"""pl_estimate_batch_dev on the device: every item of a batch whose correspondences are in device memory - fp32 or fp64,
contiguous, column or row views - carries the bits of pl_estimate_batch on the same values as doubles (model, mask, stats), and
the call goes where the host call goes (pl_last_batch_report).  The reference of every comparison is the host batch."""
import math
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from device_arrays import Allocation, DeviceArray, column_view, on_gpu, row_view
from poselib_amd import _lib as L
from poselib_amd import synth

pytestmark = pytest.mark.gpu

STAT_KEYS = ("refinements", "iterations", "num_inliers", "inlier_ratio", "model_score", "hypotheses")
KINDS = ("abs", "rel", "fund", "hom")
SCENE_SEED = {"abs": 11, "rel": 13, "fund": 17, "hom": 15}
OPENCV = [1000.0, 1000.0, 500.0, 500.0, -0.08, 0.02, 0.001, -0.0005]
WARM_H = np.array([[1.0, 0.01, 3.0], [-0.01, 1.0, -2.0], [1e-5, -1e-5, 1.0]])


def options(seed, **top):
    """short loops, but group-eligible (min_iterations <= 4096); a seed of its own per item"""
    ransac = {"max_iterations": 2000, "min_iterations": 100, "seed": seed}
    ransac.update(top.pop("ransac", {}))
    return dict(top, ransac=ransac)


def model_bytes(m):
    if hasattr(m, "pose"):  # Image
        return np.r_[m.pose.q, m.pose.t, m.camera.params].tobytes()
    if hasattr(m, "q"):
        return np.r_[m.q, m.t].tobytes()
    return np.ascontiguousarray(m, dtype=np.float64).tobytes()


def assert_same(got, want, what):
    (gm, gi), (wm, wi) = got, want
    for k in STAT_KEYS:
        assert gi[k] == wi[k], (what, k, gi[k], wi[k])
    assert gi["inliers"] == wi["inliers"], what
    assert model_bytes(gm) == model_bytes(wm), what


_SCENES = {}


def scene(kind, n, seed=None):
    """(a, b, extras) of one estimator, made once per (kind, n, seed)"""
    seed = SCENE_SEED[kind.split("_")[0]] + n if seed is None else seed
    key = (kind, n, seed)
    if key not in _SCENES:
        if kind == "abs":
            d = synth.absolute_pose_scene(n, 0.3, seed)
            _SCENES[key] = (d["p2d"], d["p3d"], d)
        elif kind == "abs_opencv":
            d = synth.absolute_pose_scene(n, 0.3, seed)
            _SCENES[key] = (synth.opencv_distort_pixels(d["p2d"], OPENCV), d["p3d"], d)
        elif kind == "rel":
            d = synth.relative_pose_scene(n, 0.3, seed)
            _SCENES[key] = (d["x1"], d["x2"], d)
        elif kind == "fund":
            d = synth.fundamental_scene(n, 0.3, seed)
            _SCENES[key] = (d["x1"], d["x2"], d)
        else:
            d = synth.homography_scene(n, 0.3, seed)
            _SCENES[key] = (d["x1"], d["x2"], d)
    return _SCENES[key]


def problem(kind, a, b, d, opt):
    if kind == "abs":
        return ("abs", a, b, d["camera"], opt)
    if kind == "abs_opencv":
        return ("abs", a, b, {"model": "OPENCV", "params": OPENCV}, opt)
    if kind == "rel":
        return ("rel", a, b, d["camera1"], d["camera2"], opt)
    return (kind, a, b, opt)


# how an item's two sets lie in device memory: name -> (upload, values are fp32)
FORMS = {
    "fp64": (lambda x: on_gpu(x), False),                             # contiguous fp64: read in place
    "fp32_columns": (lambda x: column_view(x, np.float32), True),     # NaN neighbours, a 4-byte-aligned address
    "fp64_rows": (lambda x: row_view(x, np.float64), False),          # NaN rows between
    "fp32": (lambda x: on_gpu(x, np.float32), True),                  # contiguous fp32
}


def widened(x, f32):
    return x.astype(np.float32).astype(np.float64) if f32 else x


def both_batches(specs):
    """specs: (scene kind, n, form, options[, scene seed]) per item -> (host problems, device problems)"""
    host, dev = [], []
    for spec in specs:
        kind, n, form, opt = spec[:4]
        a, b, d = scene(kind, n, *spec[4:])
        upload, f32 = FORMS[form]
        host.append(problem(kind, widened(a, f32), widened(b, f32), d, opt))
        dev.append(problem(kind, upload(a), upload(b), d, opt))
    return host, dev


def run_both(gpu, specs):
    host, dev = both_batches(specs)
    want = gpu.estimate_batch(host)
    want_report = gpu.last_batch_report()
    got = gpu.estimate_batch(dev)
    got_report = gpu.last_batch_report()
    return got, got_report, want, want_report


# ---------------------------------------------------------------- 1: sizes, one call
SIZES = (12, 63, 64, 65, 255, 256, 257, 1023, 1024, 1300)  # wave and block edges, the 1024 switches, 12 = 7-point sample + 4 + 1


def test_sizes_in_one_call(gpu):
    specs = [(kind, n, "fp64", options(100 * k + i)) for k, kind in enumerate(KINDS) for i, n in enumerate(SIZES)]
    got, got_report, want, want_report = run_both(gpu, specs)
    for spec, g, w in zip(specs, got, want):
        if spec[1] >= 255:  # the scene is solved: a degenerate one would show here, in the reference
            assert w[1]["num_inliers"] > 0.3 * spec[1], spec[:2]
        assert_same(g, w, spec[:2])
    # the device call is grouped exactly like the host call - not every item through the single _dev calls
    assert got_report == want_report
    assert got_report["grouped"] == len(specs) and got_report["solo"] == 0 and got_report["items"] == len(specs)


# ---------------------------------------------------------------- 2: ingested and in-place members in one launch
def test_mixed_forms_and_ragged_sizes_in_one_group(gpu):
    """neighbours of very different size: the grid over-provisions the small members, and every read outside a member's own rows
    meets a NaN of a column or row view"""
    sizes, forms = (12, 257, 4099, 1300), tuple(FORMS)
    specs = []
    for k, kind in enumerate(KINDS):
        for j in range(8):
            specs.append((kind, sizes[j % 4], forms[(j + j // 4) % 4], options(1000 + 10 * k + j)))
    assert {(s[1], s[2]) for s in specs if s[0] == "abs"} >= {(12, "fp64"), (12, "fp32_columns"), (4099, "fp64_rows"), (4099, "fp32")}
    got, got_report, want, want_report = run_both(gpu, specs)
    for spec, g, w in zip(specs, got, want):
        assert_same(g, w, spec[:3])
    assert got_report == want_report and got_report["grouped"] == len(specs)


# ---------------------------------------------------------------- 3: group members with special paths
def test_special_members_among_plain_ones(gpu):
    n = 300
    specs = [
        ("abs", n, "fp64", options(1)),
        ("abs_opencv", 1300, "fp32_columns", options(2)),                               # the bound comes back from k_prepare_g
        ("abs", n, "fp64_rows", options(3, ransac={"progressive_sampling": True})),     # PROSAC
        ("abs", 1300, "fp32", options(4)),
        ("hom", n, "fp64", options(5)),
        ("hom", 1300, "fp32_columns", dict(options(6), initial_model=WARM_H)),          # a warm start
        ("hom", n, "fp32", options(7)),
        ("fund", n, "fp64_rows", options(8)),
        ("fund", 1300, "fp64", options(9, real_focal_check=True)),                      # uncentred normalisation
        ("fund", n, "fp32_columns", options(10, real_focal_check=True)),
        ("rel", n, "fp32", options(11)),
    ]
    got, got_report, want, want_report = run_both(gpu, specs)
    for spec, g, w in zip(specs, got, want):
        assert_same(g, w, spec[:3])
    assert got_report == want_report and got_report["grouped"] == len(specs)


# ---------------------------------------------------------------- 4: the grouped statistics on their own
def sequential_stats(x1, x2, centroid):
    """normalize_points' two reductions (utils.cc:584-644) and the two-view bound's maximum, one addition after the other"""
    p1, p2 = x1.tolist(), x2.tolist()
    n = len(p1)
    c = [0.0, 0.0, 0.0, 0.0]
    if centroid:
        for k in range(n):
            c[0] += p1[k][0]
            c[1] += p1[k][1]
            c[2] += p2[k][0]
            c[3] += p2[k][1]
        c = [v / float(n) for v in c]
    scale = 0.0
    for k in range(n):
        a0, a1, b0, b1 = p1[k][0], p1[k][1], p2[k][0], p2[k][1]
        if centroid:
            a0, a1, b0, b1 = a0 - c[0], a1 - c[1], b0 - c[2], b1 - c[3]
        scale += math.sqrt(a0 * a0 + a1 * a1)
        scale += math.sqrt(b0 * b0 + b1 * b1)
    scale /= math.sqrt(2) * n
    m = 0.0
    for k in range(n):
        for v, ck in ((p1[k][0], c[0]), (p1[k][1], c[1]), (p2[k][0], c[2]), (p2[k][1], c[3])):
            m = max(m, abs((v - ck) / scale))
    return c, scale, m


def bits(values):
    return np.asarray(values, dtype=np.float64).tobytes()


STATS_SIZES = (7, 63, 64, 65, 255, 256, 257, 1023, 1024, 4099)


@pytest.mark.parametrize("centroid", [True, False], ids=["centred", "uncentred"])
def test_grouped_point_stats_carry_the_sequential_sums_bits(gpu, centroid):
    """all sizes in ONE launch, in-place and ingested members side by side"""
    pairs, hosts = [], []
    for i, n in enumerate(STATS_SIZES):
        x1, x2, _ = scene("fund", n)
        hosts.append((x1, x2))
        pairs.append((on_gpu(x1), on_gpu(x2)) if i % 2 == 0 else (column_view(x1, np.float64), row_view(x2, np.float64)))
    got = gpu.point_stats_group_dev(pairs, centroid)
    assert len(got) == len(STATS_SIZES)
    for n, (x1, x2), pair, g in zip(STATS_SIZES, hosts, pairs, got):
        c, scale, m = sequential_stats(x1, x2, centroid)
        assert bits(np.r_[g["c1"], g["c2"]]) == bits(c), (n, centroid)
        assert bits([g["scale"]]) == bits([scale]), (n, centroid, g["scale"], scale)
        assert bits([g["absmax_normalised"]]) == bits([m]), (n, centroid)
        assert g["absmax_first"] == np.abs(x1).max()
        single = gpu.point_stats_dev(pair[0], pair[1], centroid)  # the single-member form: the same body
        for key in ("c1", "c2", "scale", "absmax_normalised", "absmax_first"):
            assert bits(single[key]) == bits(g[key]), (n, key)


def test_grouped_point_stats_keep_a_nan_to_its_member(gpu):
    x1, x2, _ = scene("fund", 257)
    y1, y2, _ = scene("fund", 64)
    bad = x1.copy()
    bad[200, 1] = np.nan
    got = gpu.point_stats_group_dev([(on_gpu(x1), on_gpu(x2)), (on_gpu(bad), on_gpu(x2)), (on_gpu(y1), on_gpu(y2))], False)
    assert math.isnan(got[1]["absmax_first"]) and math.isnan(got[1]["absmax_normalised"]) and math.isnan(got[1]["scale"])
    for g, (p1, p2) in ((got[0], (x1, x2)), (got[2], (y1, y2))):
        c, scale, m = sequential_stats(p1, p2, False)
        assert bits([g["scale"], g["absmax_normalised"]]) == bits([scale, m]) and g["absmax_first"] == np.abs(p1).max()


# ---------------------------------------------------------------- 5: solo and unsupported routes
def test_solo_routes(gpu):
    empty = (np.zeros((0, 2)), np.zeros((0, 2)))
    six = (np.arange(12.0).reshape(6, 2), np.arange(12.0).reshape(6, 2) + 1.0)
    a, b, d = scene("rel", 300)
    f1, f2, _ = scene("fund", 300)
    items = [
        ("hom", empty[0], empty[1], options(1)),                                           # n = 0
        ("fund", six[0], six[1], options(2)),                                              # below the 7-point sample
        ("fund", f1, f2, options(3, ransac={"min_iterations": 5000, "max_iterations": 6000})),  # a long fixed-length run
        ("rel", a, b, d["camera1"], d["camera2"], options(4, tangent_sampson=True)),       # no group form
        ("fund", f1, f2, options(5)),                                                      # ... and one grouped neighbour
    ]
    want = gpu.estimate_batch(items)
    want_report = gpu.last_batch_report()
    got = gpu.estimate_batch([(p[0], on_gpu(p[1]), on_gpu(p[2])) + tuple(p[3:]) for p in items])
    report = gpu.last_batch_report()
    for i, (g, w) in enumerate(zip(got, want)):
        assert_same(g, w, i)
    assert report == want_report and report["solo"] == 4 and report["grouped"] == 1


def test_an_unsupported_item_leaves_its_neighbours_alone(gpu):
    p2, p3, d = scene("abs", 300)
    h1, h2, _ = scene("hom", 300)
    neighbours = [("abs", p2, p3, d["camera"], options(1)), ("hom", h1, h2, options(2))]
    want = gpu.estimate_batch(neighbours)
    dev = [("abs", on_gpu(p2), on_gpu(p3), d["camera"], options(1)),
           ("abs", on_gpu(p2), on_gpu(p3), d["camera"], options(3, estimate_focal_length=True)),
           ("hom", on_gpu(h1), on_gpu(h2), options(2))]
    batch = gpu.Batch(dev)
    with pytest.raises(gpu.PoseLibAmdError) as e:
        batch.run()
    assert f"error {L.PL_ERR_UNSUPPORTED}:" in str(e.value) and "item 1:" in str(e.value)
    assert [it.status for it in batch.items] == [L.PL_OK, L.PL_ERR_UNSUPPORTED, L.PL_OK]
    got = batch.results()
    assert_same(got[0], want[0], "abs neighbour")
    assert_same(got[2], want[1], "hom neighbour")


# ---------------------------------------------------------------- 6: a rejected item does not stop the rest
def test_a_rejected_item_does_not_stop_the_rest(gpu):
    specs = [("hom", 300, "fp64", options(i), 50 + i) for i in range(5)]
    host, dev = both_batches(specs)
    want = gpu.estimate_batch(host)
    x1 = np.ascontiguousarray(scene("hom", 300, 52)[0])
    pinned = DeviceArray(x1, x1.ctypes.data, Allocation(x1.nbytes, "pinned"))  # (allocated, never touched)
    dev[2] = ("hom", pinned, dev[2][2], dev[2][3])
    batch = gpu.Batch(dev)
    with pytest.raises(gpu.PoseLibAmdError) as e:
        batch.run()
    assert f"error {L.PL_ERR_INVALID}:" in str(e.value) and "item 2:" in str(e.value) and "host memory" in str(e.value)
    assert [it.status for it in batch.items] == [L.PL_OK, L.PL_OK, L.PL_ERR_INVALID, L.PL_OK, L.PL_OK]
    got = batch.results()
    for i in (0, 1, 3, 4):
        assert_same(got[i], want[i], i)


# ---------------------------------------------------------------- 7: two host threads
def test_two_host_threads_with_a_batch_each_in_flight(gpu):
    def specs_of(t):
        return [(KINDS[i % 4], (150, 300, 1100)[i % 3], tuple(FORMS)[(i + t) % 4], options(500 * t + i), 900 + 40 * t + i) for i in range(24)]

    batches = [both_batches(specs_of(t)) for t in range(2)]
    alone = [gpu.estimate_batch(dev) for _, dev in batches]
    for (host, _), res in zip(batches, alone):  # (and the batch run alone equals the host call)
        for i, (g, w) in enumerate(zip(res, gpu.estimate_batch(host))):
            assert_same(g, w, i)
    out, errors = [None, None], []

    def work(t):
        try:
            gpu.set_device(0)
            for _ in range(2):
                out[t] = gpu.estimate_batch(batches[t][1])
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for t in range(2):
        for i, (g, w) in enumerate(zip(out[t], alone[t])):
            assert_same(g, w, (t, i))


# ---------------------------------------------------------------- 8: torch
def test_views_of_one_torch_tensor_in_a_process_that_imports_torch_first(gpu):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "batch_device_torch_child.py")], capture_output=True, text=True,
                       timeout=300, cwd=root)
    if r.returncode == 0 and "torch sees no GPU" in r.stdout:
        pytest.skip("torch sees no GPU")
    assert r.returncode == 0 and "torch batch child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
