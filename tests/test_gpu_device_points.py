"""Correspondences taken from device memory (torch tensors on the GPU: float32 / float64, strided rows) give the host call's
result bit for bit: model, inlier mask, refinements, iterations, num_inliers, inlier_ratio, model_score and hypotheses.

Device input goes in front of the existing preparation (k_ingest -> the fp64 block k_prepare takes; k_ingest_soa -> a resident
problem's block; k_point_stats -> the numbers the host front-ends sum over the caller's arrays), so equality with the host call is
the whole acceptance condition.  Scenes: poselib_amd.synth with outlier_ratio 0.3.

The device arrays are tests/device_arrays.py's (allocated through the library's own HIP runtime, behind
__cuda_array_interface__); torch tensors are covered in a process of their own that imports torch first (the last test)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from device_arrays import Allocation, DeviceArray, column_view, hip, on_gpu, row_view
from poselib_amd import _lib as L
from poselib_amd import synth

pytestmark = pytest.mark.gpu

STAT_KEYS = ("refinements", "iterations", "num_inliers", "inlier_ratio", "model_score", "hypotheses")
SIZES = (7, 63, 64, 65, 255, 256, 257, 1023, 1024, 4099)  # wave edges, block edges, the 1024 switch of the two-view bound, a tail
OPENCV = [1000.0, 1000.0, 500.0, 500.0, -0.08, 0.02, 0.001, -0.0005]


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


def scene(kind, n):
    """(a, b, extras) of one estimator, made once per (kind, n)"""
    key = (kind, n)
    if key not in _SCENES:
        if kind == "abs":
            d = synth.absolute_pose_scene(n, 0.3, 11)
            _SCENES[key] = (d["p2d"], d["p3d"], d)
        elif kind == "abs_opencv":
            d = synth.absolute_pose_scene(n, 0.3, 12)
            _SCENES[key] = (synth.opencv_distort_pixels(d["p2d"], OPENCV), d["p3d"], d)
        elif kind == "rel":
            d = synth.relative_pose_scene(n, 0.3, 13)
            _SCENES[key] = (d["x1"], d["x2"], d)
        elif kind == "fund":
            d = synth.fundamental_scene(n, 0.3, 11)
            _SCENES[key] = (d["x1"], d["x2"], d)
        elif kind == "hom":
            d = synth.homography_scene(n, 0.3, 15)
            _SCENES[key] = (d["x1"], d["x2"], d)
        else:
            d = synth.radial_1d_scene(n, 0.3, 16)
            _SCENES[key] = (d["p2d"], d["p3d"], d)
    return _SCENES[key]


# every front-end case of the issue: name -> (scene kind, call(P, a, b, extras))
WARM_H = np.array([[1.0, 0.01, 3.0], [-0.01, 1.0, -2.0], [1e-5, -1e-5, 1.0]])
CASES = {
    "abs_simple_pinhole": ("abs", lambda P, a, b, d: P.estimate_absolute_pose(a, b, d["camera"], {"ransac": {"seed": 3}})),
    "abs_opencv": ("abs_opencv", lambda P, a, b, d: P.estimate_absolute_pose(a, b, {"model": "OPENCV", "params": OPENCV}, {"ransac": {"seed": 4}})),
    "rel": ("rel", lambda P, a, b, d: P.estimate_relative_pose(a, b, d["camera1"], d["camera2"], {"ransac": {"seed": 5}})),
    "rel_tangent": ("rel", lambda P, a, b, d: P.estimate_relative_pose(a, b, d["camera1"], d["camera2"],
                                                                      {"ransac": {"seed": 6}, "tangent_sampson": True})),
    "fund": ("fund", lambda P, a, b, d: P.estimate_fundamental(a, b, {"ransac": {"seed": 7}})),
    "fund_real_focal_check": ("fund", lambda P, a, b, d: P.estimate_fundamental(a, b, {"ransac": {"seed": 7}, "real_focal_check": True})),
    "hom": ("hom", lambda P, a, b, d: P.estimate_homography(a, b, {"ransac": {"seed": 8}})),
    "hom_warm": ("hom", lambda P, a, b, d: P.estimate_homography(a, b, {"ransac": {"seed": 8}}, initial_H=WARM_H)),
}
N_CASE = 1300  # above 1024: the matrix-core scorers and the two-view bound are on the path


def as_dtype_on_host(x, dtype):
    return x if dtype == np.float64 else x.astype(np.float32).astype(np.float64)


_HOST = {}


def host_result(gpu, name, n, f32):
    """the host call of a case, made once and shared"""
    key = (name, n, f32)
    if key not in _HOST:
        kind, call = CASES[name]
        a, b, d = scene(kind, n)
        if f32:
            a, b = a.astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64)
        _HOST[key] = call(gpu, a, b, d)
    return _HOST[key]


# ---------------------------------------------------------------- 1, 2: contiguous fp64 and fp32
@pytest.mark.parametrize("name", sorted(CASES))
def test_fp64_contiguous_equals_host_call(gpu, name):
    kind, call = CASES[name]
    a, b, d = scene(kind, N_CASE)
    got = call(gpu, on_gpu(a), on_gpu(b), d)
    # the scene is solved - the comparison is not between two failures: 70 % of the matches are true ones, and with 0.5 px of noise
    # per coordinate in both images a good share of those stays inside the one-pixel thresholds
    assert got[1]["num_inliers"] > 0.3 * N_CASE
    assert_same(got, host_result(gpu, name, N_CASE, False), name)


@pytest.mark.parametrize("name", sorted(CASES))
def test_fp32_equals_host_call_on_the_widened_values(gpu, name):
    kind, call = CASES[name]
    a, b, d = scene(kind, N_CASE)
    got = call(gpu, on_gpu(a, np.float32), on_gpu(b, np.float32), d)
    assert_same(got, host_result(gpu, name, N_CASE, True), name)


# ---------------------------------------------------------------- 3: views
@pytest.mark.parametrize("f32", [False, True], ids=["fp64", "fp32"])
@pytest.mark.parametrize("view", ["columns", "rows"])
@pytest.mark.parametrize("name", ["abs_simple_pinhole", "fund", "hom", "rel_tangent"])
def test_strided_views_equal_host_call(gpu, name, view, f32):
    kind, call = CASES[name]
    a, b, d = scene(kind, N_CASE)
    dtype = np.float32 if f32 else np.float64
    make = column_view if view == "columns" else row_view
    ta, tb = make(a, dtype), make(b, dtype)
    size = np.dtype(dtype).itemsize
    if view == "columns":
        assert ta.view.strides == (5 * size, size) and (ta.data_ptr - ta.allocation.ptr) == size
        assert not f32 or ta.data_ptr % 8 == 4
    else:
        assert ta.view.strides[0] == 2 * a.shape[1] * size
    assert_same(call(gpu, ta, tb, d), host_result(gpu, name, N_CASE, f32), (name, view, f32))


def test_column_stride_other_than_one_is_made_contiguous(gpu):
    kind, call = CASES["hom"]
    a, b, d = scene(kind, N_CASE)
    ta, tb = on_gpu(a.T.copy()), on_gpu(b.T.copy())
    ta, tb = DeviceArray(ta.view.T, ta.host_base, ta.allocation), DeviceArray(tb.view.T, tb.host_base, tb.allocation)  # (N, 2) views of (2, N)
    assert ta.shape == (N_CASE, 2) and ta.view.strides[1] != 8
    assert_same(call(gpu, ta, tb, d), host_result(gpu, "hom", N_CASE, False), "transposed")


def test_binding_rejections(gpu):
    a, b, d = scene("hom", N_CASE)
    ta, tb = on_gpu(a), on_gpu(b)
    with pytest.raises(ValueError):  # host and device mixed
        gpu.estimate_homography(ta, b)
    with pytest.raises(ValueError):
        gpu.estimate_homography(a, tb)
    for dtype in (np.float16, np.int32, np.int64):
        with pytest.raises(ValueError):
            gpu.estimate_homography(on_gpu(a, dtype), on_gpu(b, dtype))
    with pytest.raises(ValueError):  # sets of different length
        gpu.estimate_homography(ta, on_gpu(b[:-1]))


# ---------------------------------------------------------------- 4: sizes at the kernels' edges
@pytest.mark.parametrize("n", SIZES)
def test_front_end_sizes(gpu, n):
    for name in ("fund", "hom"):
        kind, call = CASES[name]
        a, b, d = scene(kind, n)
        got = call(gpu, column_view(a, np.float64), on_gpu(b), d)  # (one set ingested, one read in place)
        assert_same(got, host_result(gpu, name, n, False), (name, n))


@pytest.mark.parametrize("n", SIZES)
def test_problem_sizes(gpu, n):
    a, b, _ = scene("fund", n)
    opt = {"ransac": {"seed": 2}}
    host, dev = gpu.Problem(gpu.KIND_FUND, a, b), gpu.Problem(gpu.KIND_FUND, column_view(a, np.float64), on_gpu(b))
    assert dev.n == n
    assert_same(dev.run(opt), host.run(opt), n)


@pytest.mark.parametrize("n", [0, 3, 6])
def test_too_few_points_give_the_host_forms_default_stats(gpu, n):
    a, b = np.arange(2.0 * n).reshape(n, 2), np.arange(2.0 * n).reshape(n, 2) + 1.0
    ta, tb = on_gpu(a), on_gpu(b)
    assert_same(gpu.estimate_fundamental(ta, tb), gpu.estimate_fundamental(a, b), n)
    if n < 4:
        assert_same(gpu.estimate_homography(ta, tb), gpu.estimate_homography(a, b), n)
    if n == 0:
        host, dev = gpu.Problem(gpu.KIND_HOM, a, b), gpu.Problem(gpu.KIND_HOM, ta, tb)
        assert_same(dev.run(), host.run(), "empty problem")
        cam = {"model": "SIMPLE_PINHOLE", "params": [1000.0, 500.0, 500.0]}
        p3, t3 = np.zeros((0, 3)), on_gpu(np.zeros((0, 3)))
        assert_same(gpu.estimate_absolute_pose(ta, t3, cam), gpu.estimate_absolute_pose(a, p3, cam), "empty abs")
        assert_same(gpu.estimate_relative_pose(ta, tb, cam, cam), gpu.estimate_relative_pose(a, b, cam, cam), "empty rel")


# ---------------------------------------------------------------- 5: the statistics on their own
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


def numpy_stats(x1, x2):
    """the same numbers with numpy's own (pairwise) sums"""
    n = x1.shape[0]
    c = [x1[:, 0].sum() / n, x1[:, 1].sum() / n, x2[:, 0].sum() / n, x2[:, 1].sum() / n]
    da = np.sqrt((x1[:, 0] - c[0]) ** 2 + (x1[:, 1] - c[1]) ** 2)
    db = np.sqrt((x2[:, 0] - c[2]) ** 2 + (x2[:, 1] - c[3]) ** 2)
    return c, np.stack([da, db], axis=1).reshape(-1).sum() / (math.sqrt(2) * n)


def bits(values):
    return np.asarray(values, dtype=np.float64).tobytes()


@pytest.mark.parametrize("n", SIZES)
def test_point_stats_carry_the_sequential_sums_bits(gpu, n):
    x1, x2, _ = scene("fund", n)
    for centroid in (True, False):
        c, scale, m = sequential_stats(x1, x2, centroid)
        if centroid and n >= 65:  # this input tells the orders apart: numpy's pairwise sums give other bits
            c_np, scale_np = numpy_stats(x1, x2)
            assert bits(c_np) != bits(c) or bits([scale_np]) != bits([scale]), n
        for ta, tb in ((on_gpu(x1), on_gpu(x2)), (column_view(x1, np.float64), row_view(x2, np.float64))):
            got = gpu.point_stats_dev(ta, tb, centroid)
            assert bits(np.r_[got["c1"], got["c2"]]) == bits(c), (n, centroid)
            assert bits([got["scale"]]) == bits([scale]), (n, centroid, got["scale"], scale)
            assert bits([got["absmax_normalised"]]) == bits([m]), (n, centroid)
            assert got["absmax_first"] == np.abs(x1).max()


def test_point_stats_propagate_a_nan(gpu):
    x1, x2, _ = scene("fund", 257)
    x1 = x1.copy()
    x1[200, 1] = np.nan
    got = gpu.point_stats_dev(on_gpu(x1), on_gpu(x2), False)
    assert math.isnan(got["absmax_first"]) and math.isnan(got["absmax_normalised"]) and math.isnan(got["scale"])


# ---------------------------------------------------------------- 6: resident problems
def problem_inputs(kind_id, n):
    """points at the level pl_problem_create takes them, with a threshold that suits them"""
    if kind_id == 0:
        a, b, d = scene("abs", n)
        return (a - 500.0) / 1000.0, b, {"max_error": 12.0 / 1000.0, "ransac": {"seed": 1}}
    if kind_id == 1:
        a, b, d = scene("rel", n)
        return (a - 500.0) / 1000.0, (b - 500.0) / 1000.0, {"max_error": 1.0 / 1000.0, "ransac": {"seed": 1}}
    if kind_id == 2:
        a, b, d = scene("fund", n)
        return a, b, {"max_error": 1.0, "ransac": {"seed": 1}}
    if kind_id == 3:
        a, b, d = scene("hom", n)
        return a, b, {"max_error": 1.0, "ransac": {"seed": 1}}
    a, b, d = scene("rad1d", n)
    return a, b, {"max_error": 12.0, "ransac": {"seed": 1}}


@pytest.mark.parametrize("f32", [False, True], ids=["fp64", "fp32"])
@pytest.mark.parametrize("kind_id", [0, 1, 2, 3, 5])
def test_resident_problem_equals_host_created(gpu, kind_id, f32):
    a, b, opt = problem_inputs(kind_id, N_CASE)
    dtype = np.float32 if f32 else np.float64
    ha, hb = as_dtype_on_host(a, dtype), as_dtype_on_host(b, dtype)
    host = gpu.Problem(kind_id, ha, hb)
    dev = gpu.Problem(kind_id, column_view(a, dtype), row_view(b, dtype))
    want = host.run(opt)
    assert want[1]["num_inliers"] > 0.3 * N_CASE
    got = dev.run(opt)
    assert_same(got, want, kind_id)
    model = want[0]
    assert dev.score(model, opt["max_error"]) == host.score(model, opt["max_error"])
    assert np.array_equal(gpu.inlier_mask(dev, model, opt["max_error"]), gpu.inlier_mask(host, model, opt["max_error"]))


def test_tangent_problem_equals_host_created(gpu):
    a, b, d = scene("rel", N_CASE)
    opt = {"max_error": 1.0, "ransac": {"seed": 9}}
    host = gpu.TangentProblem(a, b, d["camera1"], d["camera2"])
    want = host.run(opt)
    for f32 in (False, True):
        dtype = np.float32 if f32 else np.float64
        ref = want if not f32 else gpu.TangentProblem(as_dtype_on_host(a, dtype), as_dtype_on_host(b, dtype), d["camera1"],
                                                      d["camera2"]).run(opt)
        dev = gpu.TangentProblem(column_view(a, dtype), on_gpu(b, dtype), d["camera1"], d["camera2"])
        assert_same(dev.run(opt), ref, ("tangent", f32))


def test_ransac_batch_over_device_and_host_created_problems(gpu):
    problems, opts, singles = [], [], []
    for kind_id in (0, 1, 2, 3):
        for n in (700, 1300):
            a, b, opt = problem_inputs(kind_id, n)
            host = gpu.Problem(kind_id, a, b)
            dev = gpu.Problem(kind_id, on_gpu(a), column_view(b, np.float64))
            want = host.run(opt)
            problems += [dev, host]
            opts += [opt, opt]
            singles += [want, want]
    got = gpu.ransac_batch(problems, opts)
    report = gpu.last_batch_report()
    assert report["grouped"] == len(problems), report
    for i, (g, w) in enumerate(zip(got, singles)):
        assert_same(g, w, i)


# ---------------------------------------------------------------- 7: rejections that need the device (no kernel is launched)
def test_device_dependent_rejections(gpu):
    t = on_gpu(scene("hom", N_CASE)[0])
    good = L.DevicePoints(t.data_ptr, 2, L.PL_F64, 2)
    assert gpu.check_device_points(good, N_CASE, 2) == L.PL_OK
    host = np.zeros((N_CASE, 2))
    assert gpu.check_device_points(L.DevicePoints(host.ctypes.data, 2, L.PL_F64, 2), N_CASE, 2) == L.PL_ERR_INVALID
    assert b"device points" in L.lib().pl_last_error()
    assert gpu.check_device_points(L.DevicePoints(t.data_ptr + 1, 2, L.PL_F64, 2), N_CASE, 2) == L.PL_ERR_INVALID
    for kind in ("pinned", "managed"):  # (allocated, never touched)
        other = Allocation(16 * N_CASE, kind)
        assert gpu.check_device_points(L.DevicePoints(other.ptr, 2, L.PL_F64, 2), N_CASE, 2) == L.PL_ERR_INVALID, kind
        assert (b"managed" if kind == "managed" else b"host") in L.lib().pl_last_error()
    # rows that reach beyond the allocation
    assert gpu.check_device_points(good, 1 << 30, 2) == L.PL_ERR_INVALID
    assert b"beyond the allocation" in L.lib().pl_last_error()
    assert gpu.check_device_points(L.DevicePoints(t.data_ptr, 4, L.PL_F64, 2), N_CASE, 2) == L.PL_ERR_INVALID  # (twice the rows' reach)


def test_memory_of_another_device_is_rejected(gpu):
    if gpu.device_count() < 2:
        pytest.skip("one device visible")
    assert hip().hipSetDevice(1) == 0
    try:
        other = Allocation(16 * N_CASE)
    finally:
        assert hip().hipSetDevice(0) == 0
    assert gpu.check_device_points(L.DevicePoints(other.ptr, 2, L.PL_F64, 2), N_CASE, 2) == L.PL_ERR_INVALID
    assert b"another device" in L.lib().pl_last_error()


def test_estimate_focal_length_is_unsupported_from_device_memory(gpu):
    a, b, d = scene("abs", N_CASE)
    with pytest.raises(gpu.PoseLibAmdError) as e:
        gpu.estimate_absolute_pose(on_gpu(a), on_gpu(b), d["camera"], {"estimate_focal_length": True})
    assert f"error {L.PL_ERR_UNSUPPORTED}:" in str(e.value)


def test_torch_tensors_in_a_process_that_imports_torch_first(gpu):
    """torch brings a HIP runtime of its own; imported first, the library shares it and the tensors' memory is known to it.  One
    child process: float32 / float64 tensors, column and row views, a resident problem, the binding's rejections."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "device_points_torch_child.py")], capture_output=True, text=True,
                       timeout=300, cwd=root)
    assert r.returncode == 0 and "torch child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
