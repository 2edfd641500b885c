"""Matches ranked by a matcher's confidences, the part that needs no device:
  1. the rule itself (poselib_amd.score_order, the numpy statement of include/poselib_amd.h) against a sort written another way;
  2. the surface - the new symbols are declared, exported and bound, the scores descriptor gets the points' checks before the
     device is touched, and the Python host path (scores= with host arrays) is the plain call on a[order], b[order] with the mask
     scattered back: equal where a device computes, failing exactly as the plain call where none is;
  3. the intended use, on the oracle alone: with progressive_sampling, rows ranked by a confidence that is higher on inliers stop
     the loop in fewer iterations than the unranked rows, and find the same inliers."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import oracle_lib as O
import poselib_amd
from poselib_amd import _lib as L
from poselib_amd import api, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["pl_estimate_dev_scored", "pl_estimate_batch_dev_scored", "pl_debug_rank_scores", "pl_debug_rank_tile"]
FAR = 0x7F0000001000  # an address nothing dereferences
HAVE_DEVICE = poselib_amd.device_count() > 0


# ------------------------------------------------------------------------------------------ 1: the rule
def by_comparison(scores, min_score):
    """the rule as a sort on (descending score, ascending row) over python floats - no argsort, no negation of an array"""
    s = [float(v) for v in scores]
    kept = [i for i, v in enumerate(s) if v >= min_score]
    return sorted(kept, key=lambda i: (-s[i], i))


RULE_CASES = {
    "ties": [0.5, 0.25, 0.5, 0.75, 0.25, 0.5],
    "all_equal": [0.125] * 9,
    "signed_zeros": [0.0, -0.0, 1.0, -0.0, 0.0, -1.0],
    "infinities": [1.0, np.inf, -np.inf, 0.0, np.inf, -np.inf, -5.0],
    "nans": [np.nan, 0.5, np.nan, 0.25, 0.5, np.nan],
    "all_nan": [np.nan] * 4,
    "empty": [],
    "one": [3.0],
}


@pytest.mark.parametrize("name", sorted(RULE_CASES))
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_rule(name, dtype):
    s = np.array(RULE_CASES[name], dtype=dtype)
    for m in (None, -np.inf, 0.0, -0.0, 0.25, 0.3, 0.5, np.inf):  # (0.25 and 0.5 are tied values of several cases)
        got = api.score_order(s, m)
        assert got.tolist() == by_comparison(s, -np.inf if m is None else m), (name, m)
        assert not np.isnan(s[got]).any()
    # default threshold: every non-NaN row, -inf included; +inf first
    full = api.score_order(s)
    assert len(full) == int((~np.isnan(s)).sum())
    if name == "infinities":
        assert full.tolist() == [1, 4, 0, 3, 6, 2, 5]
        assert api.score_order(s, -1e308).tolist() == [1, 4, 0, 3, 6]  # -inf is kept only by a threshold of -inf
    if name == "signed_zeros":
        assert full.tolist() == [2, 0, 1, 3, 4, 5]  # -0.0 == 0.0: row order decides


def test_the_rule_on_fp32_values_and_the_same_values_as_doubles():
    rng = np.random.default_rng(5)
    s32 = (rng.integers(0, 40, 500) / np.float32(7.0)).astype(np.float32)
    s32[rng.integers(0, 500, 20)] = np.nan
    s32[:8] = np.float32(2.0 ** -149) * np.arange(-4, 4, dtype=np.float32)  # denormals
    s64 = s32.astype(np.float64)
    for m in (None, float(s32[100]), 0.1, float(np.float32(0.1))):  # (0.1 is no fp32 value: the comparison is made in doubles)
        assert api.score_order(s32, m).tolist() == api.score_order(s64, m).tolist() == by_comparison(s64, -np.inf if m is None else m)
    with pytest.raises(ValueError):
        api.score_order(s32, float("nan"))
    with pytest.raises(ValueError):
        api.score_order(np.zeros((3, 2)))


# ------------------------------------------------------------------------------------------ 2: the surface
def test_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "poselib_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(pl_[a-z0-9_]+)\s*\(", text))
    poselib_amd.build()
    lib = L.lib()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in L.EXPORTED_SYMBOLS, name
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is C.c_int, name
    assert "pl_device_scores" in text
    assert re.search(r"#define\s+PL_ABI_VERSION\s+5\b", text) and lib.pl_abi_version() == 5 and L.ABI_VERSION == 5
    assert C.sizeof(L.DeviceScores) == 32
    assert (L.DeviceScores.data.offset, L.DeviceScores.stride.offset, L.DeviceScores.dtype.offset, L.DeviceScores.min_score.offset) == (0, 8, 16, 24)
    for name in ("score_order", "rank_scores", "rank_tile"):
        assert hasattr(poselib_amd, name), name


def _scores(data=FAR, stride=1, dtype=L.PL_F32, min_score=-math.inf):
    return L.DeviceScores(data, stride, dtype, 0, min_score)


BAD_SCORES = {
    "stride (elements) is below 1": dict(stride=0),
    "dtype must be": dict(dtype=2),
    "data is null": dict(data=None),
    "not aligned": dict(data=FAR + 4, dtype=L.PL_F64),
    "min_score is NaN": dict(min_score=math.nan),
}


def _rank(desc, n=10):
    ns, order, kept = (C.c_size_t * 1)(n), np.zeros(max(n, 1), dtype=np.uint32), (C.c_size_t * 1)()
    return L.lib().pl_debug_rank_scores(None if desc is None else C.byref(desc), ns, 1, order.ctypes.data, kept)


@pytest.mark.parametrize("cause", sorted(BAD_SCORES))
def test_a_bad_scores_descriptor_is_refused_before_the_device(cause):
    assert _rank(_scores(**BAD_SCORES[cause])) == L.PL_ERR_INVALID
    msg = L.lib().pl_last_error().decode()
    assert "device scores" in msg and cause in msg, msg


def _single(kind, scores, n=100, cols_b=None, opt_edit=None):
    lib = L.lib()
    o = L.RobustOptions()
    lib.pl_default_robust_options(C.byref(o), kind)
    if opt_edit:
        opt_edit(o)
    cam = api.Camera("SIMPLE_PINHOLE", [1000.0, 500.0, 500.0])._c()
    cb = cols_b or (3 if kind == 0 else 2)
    a, b = L.DevicePoints(FAR, 2, L.PL_F64, 2), L.DevicePoints(FAR, cb, L.PL_F64, cb)
    model, st, inl, used = np.zeros(9), L.RansacStats(), np.zeros(n, dtype=np.uint8), C.c_size_t(7)
    rc = lib.pl_estimate_dev_scored(kind, C.byref(a), C.byref(b), None if scores is None else C.byref(scores), n, C.byref(o),
                                    C.byref(cam) if kind < 2 else None, C.byref(cam) if kind == 1 else None, model.ctypes.data,
                                    inl.ctypes.data, C.byref(st), C.byref(used))
    return rc, lib.pl_last_error().decode()


def test_the_single_scored_call_checks_in_the_order_of_the_plain_call():
    # what needs no device comes first, whether or not there is one
    for kind in range(4):
        rc, msg = _single(kind, _scores(stride=0))
        assert rc == L.PL_ERR_INVALID and "device scores" in msg, (kind, msg)
        rc, msg = _single(kind, None)
        assert rc == L.PL_ERR_INVALID and "descriptor is null" in msg, (kind, msg)
        rc, msg = _single(kind, _scores(), cols_b=5 - (3 if kind == 0 else 2))  # the points' own checks still speak, first
        assert rc == L.PL_ERR_INVALID and "device points" in msg, (kind, msg)
    assert _single(7, _scores())[0] == L.PL_ERR_INVALID
    # what the plain entry refuses, the scored one refuses the same way - before it looks at points or scores
    def focal(o):
        o.estimate_focal_length = 1
    rc, msg = _single(0, _scores(stride=0), opt_edit=focal)
    assert rc == L.PL_ERR_UNSUPPORTED and "estimate_focal_length" in msg, msg
    # a plausible call: the device is asked for (and a machine that has one does not know the address)
    rc, msg = _single(2, _scores())
    assert rc == (L.PL_ERR_INVALID if HAVE_DEVICE else L.PL_ERR_NO_DEVICE), msg


def test_the_batch_names_the_item_whose_scores_are_bad():
    lib = L.lib()
    count, n = 4, 50
    items, scores, used = (L.BatchItemDev * count)(), (L.DeviceScores * count)(), (C.c_size_t * count)()
    keep = []
    for i, it in enumerate(items):
        o = L.RobustOptions()
        lib.pl_default_robust_options(C.byref(o), 3)
        model, st, inl = np.zeros(9), L.RansacStats(), np.zeros(n, dtype=np.uint8)
        it.kind, it.n = 3, n
        it.a, it.b = L.DevicePoints(FAR, 2, L.PL_F64, 2), L.DevicePoints(FAR, 2, L.PL_F64, 2)
        it.opt, it.model, it.inliers, it.stats = C.pointer(o), model.ctypes.data, inl.ctypes.data, C.pointer(st)
        keep.append((o, model, st, inl))
        if i != 1:  # (item 1 is a plain item: no data)
            scores[i] = _scores()
    scores[2] = _scores(stride=-3)
    assert lib.pl_estimate_batch_dev_scored(items, scores, used, count, 4) == L.PL_ERR_INVALID
    msg = lib.pl_last_error().decode()
    if HAVE_DEVICE:  # (every address here is host memory to a device: the call reports its FIRST failing item)
        assert "item 0:" in msg and "device points" in msg, msg
    else:
        assert "item 2:" in msg and "device scores" in msg, msg
    assert items[2].status == L.PL_ERR_INVALID
    other = L.PL_ERR_INVALID if HAVE_DEVICE else L.PL_ERR_NO_DEVICE  # (with a device: the addresses are not device memory)
    assert [items[i].status for i in (0, 1, 3)] == [other] * 3
    assert lib.pl_estimate_batch_dev_scored(None, None, None, 0, 4) == L.PL_OK


class FakeDeviceArray:
    """__cuda_array_interface__ over a numpy buffer, whose address stands in for a device address; nothing dereferences it"""

    def __init__(self, array):
        self.array = array
        self.shape = array.shape

    @property
    def __cuda_array_interface__(self):
        a = self.array
        return {"shape": a.shape, "typestr": a.dtype.str, "data": (a.__array_interface__["data"][0], False),
                "strides": None if a.flags.c_contiguous else tuple(a.strides), "version": 3}


def test_python_builds_the_scores_descriptors():
    t = np.zeros((3, 40, 5), dtype=np.float32)
    base = t.__array_interface__["data"][0]
    problems = [("hom", FakeDeviceArray(t[i, :, :2]), FakeDeviceArray(t[i, :, 2:4]),
                 {"ransac": {"seed": i}, "scores": FakeDeviceArray(t[i, :, 4]), "min_score": 0.25} if i != 1 else None) for i in range(3)]
    b = api.Batch(problems)
    assert b.on_device and b.scored
    for i in (0, 2):
        s = b.scores[i]
        assert (s.data, s.stride, s.dtype, s.min_score) == (base + i * 40 * 20 + 16, 5, L.PL_F32, 0.25)
    assert not b.scores[1].data  # a plain item
    with pytest.raises(ValueError):  # device points, host scores
        api.Batch([("hom", FakeDeviceArray(t[0, :, :2]), FakeDeviceArray(t[0, :, 2:4]), {"scores": np.zeros(40)})])
    with pytest.raises(ValueError):  # host points, device scores
        api.estimate_homography(np.zeros((40, 2)), np.zeros((40, 2)), scores=FakeDeviceArray(t[0, :, 4]))
    with pytest.raises(ValueError):  # another length
        api.Batch([("hom", FakeDeviceArray(t[0, :, :2]), FakeDeviceArray(t[0, :, 2:4]), {"scores": FakeDeviceArray(t[0, :30, 4])})])
    with pytest.raises(ValueError):
        api.estimate_homography(np.zeros((40, 2)), np.zeros((40, 2)), min_score=0.5)  # a threshold without scores
    with pytest.raises(ValueError):
        api.rank_scores(np.zeros(5))  # host scores: score_order


def _outcome(call):
    try:
        return "ok", call()
    except poselib_amd.PoseLibAmdError as e:
        return "error", str(e)


HOST_CALLS = {
    "abs": lambda d, a, b, **kw: api.estimate_absolute_pose(a, b, d["camera"], {"ransac": {"seed": 2, "progressive_sampling": True}}, **kw),
    "rel": lambda d, a, b, **kw: api.estimate_relative_pose(a, b, d["camera1"], d["camera2"], {"ransac": {"seed": 2}}, **kw),
    "fund": lambda d, a, b, **kw: api.estimate_fundamental(a, b, {"ransac": {"seed": 2, "progressive_sampling": True}}, **kw),
    "hom": lambda d, a, b, **kw: api.estimate_homography(a, b, {"ransac": {"seed": 2}}, **kw),
}


def _model_bytes(m):
    if hasattr(m, "pose"):
        return np.r_[m.pose.q, m.pose.t, m.camera.params].tobytes()
    if hasattr(m, "q"):
        return np.r_[m.q, m.t].tobytes()
    return np.ascontiguousarray(m, dtype=np.float64).tobytes()


@pytest.mark.parametrize("kind", sorted(HOST_CALLS))
def test_host_scores_are_the_plain_call_on_the_ranked_rows(kind):
    n = 200
    d = {"abs": synth.absolute_pose_scene, "rel": synth.relative_pose_scene, "fund": synth.fundamental_scene,
         "hom": synth.homography_scene}[kind](n, 0.4, 77)
    a, b = (d["p2d"], d["p3d"]) if kind == "abs" else (d["x1"], d["x2"])
    rng = np.random.default_rng(9)
    scores = (d["inlier_gt"] + 0.4 * rng.standard_normal(n)).astype(np.float32)
    scores[::17] = np.nan
    order = api.score_order(scores, 0.2)
    assert 20 < len(order) < n
    status, want = _outcome(lambda: HOST_CALLS[kind](d, a[order], b[order]))
    got_status, got = _outcome(lambda: HOST_CALLS[kind](d, a, b, scores=scores, min_score=0.2))
    assert got_status == status
    if status == "error":  # no device: the scored call fails exactly as the plain one
        assert got == want and not HAVE_DEVICE
        return
    (wm, wi), (gm, gi) = want, got
    assert _model_bytes(gm) == _model_bytes(wm)
    mask = np.zeros(n, dtype=bool)
    mask[order] = wi["inliers"]
    assert gi["inliers"] == mask.tolist() and gi["n_used"] == len(order) and wi["n_used"] == len(order)
    for k in ("refinements", "iterations", "num_inliers", "inlier_ratio", "model_score"):
        assert gi[k] == wi[k], k
    # ... and in a batch
    item = {"abs": lambda a_, b_, o: ("abs", a_, b_, d["camera"], o), "rel": lambda a_, b_, o: ("rel", a_, b_, d["camera1"], d["camera2"], o)}
    make = item.get(kind, lambda a_, b_, o: (kind, a_, b_, o))
    (bm, bi), = api.estimate_batch([make(a, b, {"ransac": {"seed": 2}, "scores": scores, "min_score": 0.2})])
    (pm, pi), = api.estimate_batch([make(a[order], b[order], {"ransac": {"seed": 2}})])
    mask[:] = False
    mask[order] = pi["inliers"]
    assert _model_bytes(bm) == _model_bytes(pm) and bi["inliers"] == mask.tolist() and bi["n_used"] == len(order)


# ------------------------------------------------------------------------------------------ 3: the intended use, on the oracle
# n = 400, 70 % outliers, a confidence of 1 on inliers and 0 on outliers plus N(0, 0.35) noise.  Scene and noise seeds are fixed;
# the condition below is one on these inputs, checked on the oracle alone.
# The reference's loop ends at max(min_iterations, the dynamic bound of the best inlier ratio so far): with the default
# dyn_num_trials_mult = 3 that bound - the same for both orders, it depends on the inlier ratio alone - lies far beyond the
# iteration at which either run finds its model, and ranking changes nothing (measured: 1029 / 1029 iterations for "abs").  Ranking
# pays where FINDING the model is what takes the time, i.e. for a caller who has lowered the bound; the options below do
# (dyn_num_trials_mult = 0.002, min_iterations = 1), so a run ends soon after its first good model.
ORACLE_SEED = {"abs": 21, "rel": 22, "fund": 24, "hom": 24}
ORACLE_OPT = {"ransac": {"seed": 1, "progressive_sampling": True, "min_iterations": 1, "max_iterations": 100000,
                         "dyn_num_trials_mult": 0.002}}
INLIER_TOLERANCE = 0.05  # the two runs end in models fitted to different samples: up to 5 % of the inliers may differ at the threshold


def _oracle(kind, d, a, b, opt):
    if kind == "abs":
        return O.estimate_absolute_pose(a, b, d["camera"], opt)
    if kind == "rel":
        return O.estimate_relative_pose(a, b, d["camera1"], d["camera2"], opt)
    return (O.estimate_fundamental if kind == "fund" else O.estimate_homography)(a, b, opt)


@pytest.mark.parametrize("kind", sorted(ORACLE_SEED))
def test_ranked_rows_stop_prosac_sooner_on_the_oracle(kind):
    n = 400
    d = {"abs": synth.absolute_pose_scene, "rel": synth.relative_pose_scene, "fund": synth.fundamental_scene,
         "hom": synth.homography_scene}[kind](n, 0.7, ORACLE_SEED[kind])
    a, b = (d["p2d"], d["p3d"]) if kind == "abs" else (d["x1"], d["x2"])
    rng = np.random.default_rng(100 + ORACLE_SEED[kind])
    scores = d["inlier_gt"].astype(np.float64) + 0.35 * rng.standard_normal(n)
    order = api.score_order(scores)
    assert len(order) == n
    opt = ORACLE_OPT
    _, mask_plain, st_plain = _oracle(kind, d, a, b, opt)
    _, mask_ranked, st_ranked = _oracle(kind, d, a[order], b[order], opt)
    back = np.zeros(n, dtype=bool)
    back[order] = mask_ranked
    print(kind, "iterations unranked", st_plain["iterations"], "ranked", st_ranked["iterations"], "inliers", int(mask_plain.sum()),
          int(back.sum()), "differ", int((back != mask_plain).sum()))
    assert st_ranked["iterations"] < st_plain["iterations"]
    assert mask_plain.sum() > 0.15 * n  # the scene is solved (30 % are inliers; the planar scene's threshold keeps ~20 %)
    assert (back != mask_plain).sum() <= INLIER_TOLERANCE * mask_plain.sum()
