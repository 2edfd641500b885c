"""pl_estimate_shared_focal_relative_pose_batch_dev, the part that needs no device: the entry point, its record and the grouped
diagnostic are declared, exported and bound; an item is answered before the device is touched, with its index in the message and
the status its single call would give; SharedFocalBatch turns the views of a matcher's tensor into pl_shared_focal_item_dev
records and refuses what the call does not take.  No compute calls are made here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import poselib_amd
from poselib_amd import _lib as L
from poselib_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["pl_estimate_shared_focal_relative_pose_batch_dev", "pl_debug_point_stats_about_group_dev"]
FAR = 0x7F0000001000  # an address nothing dereferences
no_gpu = pytest.mark.skipif(poselib_amd.device_count() > 0, reason="GPU present")


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
    assert "pl_shared_focal_item_dev" in text
    # new symbols, no record changed: the layout version stays
    assert re.search(r"#define\s+PL_ABI_VERSION\s+5\b", text) and lib.pl_abi_version() == 5 and L.ABI_VERSION == 5
    for name in ("SharedFocalBatch", "estimate_shared_focal_relative_pose_batch", "point_stats_about_group_dev"):
        assert hasattr(poselib_amd, name), name


def test_item_layout():
    """status, reserved, two 24-byte descriptors by value, n, pp[2], five pointers"""
    S = L.SharedFocalItemDev
    assert (S.status.offset, S.reserved.offset, S.x1.offset, S.x2.offset, S.n.offset, S.pp.offset) == (0, 4, 8, 32, 56, 64)
    assert [getattr(S, k).offset for k in ("opt", "pose", "focal", "inliers", "stats")] == [80, 88, 96, 104, 112]
    assert C.sizeof(S) == 120


def _desc(data=FAR, row_stride=2, dtype=L.PL_F64, cols=2):
    return L.DevicePoints(data, row_stride, dtype, cols)


class _Items:
    """`count` plausible items (descriptors of addresses nothing reads), outputs kept alive"""

    def __init__(self, count, n=100):
        self.items = (L.SharedFocalItemDev * count)()
        self.scores = (L.DeviceScores * count)()
        self.masks = (L.DeviceMask * count)()
        self.n_used = (C.c_size_t * count)()
        self.keep = []
        for it in self.items:
            o = L.RobustOptions()
            L.lib().pl_default_robust_options(C.byref(o), 1)
            pose, focal, st, inl = L.CameraPose(), C.c_double(1.0), L.RansacStats(), np.zeros(n, dtype=np.uint8)
            it.x1, it.x2, it.n = _desc(), _desc(), n
            it.pp[0], it.pp[1] = 500.0, 400.0
            it.opt, it.pose, it.focal = C.pointer(o), C.pointer(pose), C.pointer(focal)
            it.inliers, it.stats = inl.ctypes.data, C.pointer(st)
            self.keep.append((o, pose, focal, st, inl))

    def run(self, scores=False, masks=False):
        return L.lib().pl_estimate_shared_focal_relative_pose_batch_dev(self.items, self.scores if scores else None,
                                                                        self.masks if masks else None, self.n_used, len(self.items), 4)


# the BAD table of tests/test_batch_device_surface.py
BAD = {
    "row_stride below cols": dict(row_stride=1),
    "unknown dtype": dict(dtype=2),
    "misaligned fp64": dict(data=FAR + 4),
}
BAD_SCORES = {
    "stride below 1": L.DeviceScores(FAR, 0, L.PL_F64, 0, 0.0),
    "unknown dtype": L.DeviceScores(FAR, 1, 2, 0, 0.0),
    "misaligned fp64": L.DeviceScores(FAR + 4, 1, L.PL_F64, 0, 0.0),
    "NaN min_score": L.DeviceScores(FAR, 1, L.PL_F32, 0, float("nan")),
}
BAD_MASKS = {"stride below 1": L.DeviceMask(FAR, 0)}


def _others_would_have_run(b, k):
    assert all(b.items[i].status == L.PL_ERR_NO_DEVICE for i in range(len(b.items)) if i != k)


@no_gpu
def test_nothing_to_do_and_null_items():
    lib = L.lib()
    assert lib.pl_estimate_shared_focal_relative_pose_batch_dev(None, None, None, None, 0, 4) == L.PL_OK
    assert lib.pl_estimate_shared_focal_relative_pose_batch_dev(None, None, None, None, 3, 4) == L.PL_ERR_INVALID
    assert _Items(5).run() == L.PL_ERR_NO_DEVICE  # (a plausible call needs the device)


@no_gpu
@pytest.mark.parametrize("case", sorted(BAD))
@pytest.mark.parametrize("which", ["x1", "x2"])
@pytest.mark.parametrize("k", [0, 3, 6])
def test_a_bad_point_descriptor_is_named_by_its_item_before_the_device(case, which, k):
    b = _Items(7)
    setattr(b.items[k], which, _desc(**BAD[case]))
    assert b.run() == L.PL_ERR_INVALID
    msg = L.lib().pl_last_error().decode()
    assert f"item {k}:" in msg and "device points" in msg, msg
    assert b.items[k].status == L.PL_ERR_INVALID
    _others_would_have_run(b, k)


@no_gpu
@pytest.mark.parametrize("k", [0, 3, 6])
def test_bad_scores_and_masks_are_named_by_their_item_before_the_device(k):
    for case, d in BAD_SCORES.items():
        b = _Items(7)
        b.scores[k] = d
        b.scores[(k + 1) % 7] = L.DeviceScores(FAR, 5, L.PL_F32, 0, 0.25)  # (a good one next to it; the rest: plain items)
        assert b.run(scores=True) == L.PL_ERR_INVALID, case
        msg = L.lib().pl_last_error().decode()
        assert f"item {k}:" in msg and "device scores" in msg, (case, msg)
        assert b.items[k].status == L.PL_ERR_INVALID
        _others_would_have_run(b, k)
    for case, d in BAD_MASKS.items():
        b = _Items(7)
        b.masks[k] = d
        assert b.run(masks=True) == L.PL_ERR_INVALID, case
        msg = L.lib().pl_last_error().decode()
        assert f"item {k}:" in msg and "device mask" in msg, (case, msg)
        assert b.items[k].status == L.PL_ERR_INVALID
        _others_would_have_run(b, k)


def _single_status(it):
    """what pl_estimate_shared_focal_relative_pose_dev says of the same arguments"""
    return L.lib().pl_estimate_shared_focal_relative_pose_dev(C.byref(it.x1), C.byref(it.x2), None, it.n, C.cast(it.pp, C.c_void_p),
                                                              it.opt, it.pose, it.focal, it.inliers, None, it.stats, None)


@no_gpu
@pytest.mark.parametrize("field", ["opt", "pose", "focal", "rejected option"])
def test_null_arguments_and_rejected_options_get_the_single_calls_status(field):
    k = 2
    b = _Items(5)
    if field == "rejected option":
        b.keep[k][0].min_fov = float("nan")  # (validate_options: the record was not filled)
    else:
        setattr(b.items[k], field, None)
    want = _single_status(b.items[k])
    cause = L.lib().pl_last_error().decode()
    assert want == L.PL_ERR_INVALID  # (before the device, as the single call)
    assert b.run() == want
    msg = L.lib().pl_last_error().decode()
    assert f"item {k}: {cause}" in msg, (msg, cause)
    assert b.items[k].status == want
    _others_would_have_run(b, k)


class FakeDeviceArray:
    """__cuda_array_interface__ over a numpy buffer, whose address stands in for a device address; nothing dereferences it"""

    def __init__(self, array):
        self.array = array

    @property
    def __cuda_array_interface__(self):
        a = self.array
        return {"shape": a.shape, "typestr": a.dtype.str, "data": (a.__array_interface__["data"][0], False),
                "strides": None if a.flags.c_contiguous else tuple(a.strides), "version": 3}


def test_the_batch_builds_its_records_from_views_of_one_tensor():
    """the views of a padded (pairs, N, 5) float32 tensor: pointer, stride and dtype of both sets and of the scores column"""
    t = np.zeros((3, 50, 5), dtype=np.float32)
    base = t.__array_interface__["data"][0]
    pairs = [(FakeDeviceArray(t[i, :, :2]), FakeDeviceArray(t[i, :, 2:4]), (320.0 + i, 240.0),
              {"ransac": {"seed": i}, "scores": FakeDeviceArray(t[i, :, 4]), "min_score": 0.25}) for i in range(3)]
    b = api.SharedFocalBatch(pairs)
    assert isinstance(b.items[0], L.SharedFocalItemDev) and len(b.keep) == 3 and b.scored and not b.masked
    for i in range(3):
        it, row = b.items[i], base + i * 50 * 20
        assert (it.x1.data, it.x1.row_stride, it.x1.dtype, it.x1.cols) == (row, 5, L.PL_F32, 2)
        assert (it.x2.data, it.x2.row_stride, it.x2.dtype, it.x2.cols) == (row + 8, 5, L.PL_F32, 2)
        s = b.scores[i]
        assert (s.data, s.stride, s.dtype, s.min_score) == (row + 16, 5, L.PL_F32, 0.25)
        assert (it.pp[0], it.pp[1], it.n) == (320.0 + i, 240.0, 50)
        o = it.opt.contents
        assert o.ransac.seed == i and o.ransac.score_initial_model == 0
        assert it.pose and it.focal and it.inliers and it.stats and it.focal.contents.value == 1.0
    assert len(b.n_used) == 3
    # a warm start travels in the record's pose and focal length
    start = api.ImagePair(api.CameraPose([0.0, 1.0, 0.0, 0.0], [1.0, 2.0, 3.0]), api.Camera("SIMPLE_PINHOLE", [700.0, 320.0, 240.0]))
    b = api.SharedFocalBatch([(pairs[0][0], pairs[0][1], (320.0, 240.0), {"initial_pair": start})])
    it = b.items[0]
    assert it.opt.contents.ransac.score_initial_model == 1 and it.focal.contents.value == 700.0 and list(it.pose.contents.t) == [1.0, 2.0, 3.0]
    assert not b.scored and b.scores[0].data is None


def test_what_the_batch_refuses():
    dev = lambda *shape: FakeDeviceArray(np.zeros(shape))  # noqa: E731
    host = np.zeros((8, 2))
    pp = (0.0, 0.0)
    with pytest.raises(ValueError, match="estimate_batch"):  # host arrays: the host batch serves them
        api.SharedFocalBatch([(host, host, pp, None)])
    with pytest.raises(ValueError, match="estimate_batch"):
        api.estimate_shared_focal_relative_pose_batch([(dev(8, 2), dev(8, 2), pp, None), (host, host, pp, None)])
    with pytest.raises(ValueError, match="same way"):  # mixed sets
        api.SharedFocalBatch([(dev(8, 2), host, pp, None)])
    with pytest.raises(ValueError, match="differ in length"):
        api.SharedFocalBatch([(dev(8, 2), dev(9, 2), pp, None)])
    with pytest.raises(ValueError, match="7 scores for 8"):
        api.SharedFocalBatch([(dev(8, 2), dev(8, 2), pp, {"scores": dev(7)})])
    with pytest.raises(ValueError, match="min_score without scores"):
        api.SharedFocalBatch([(dev(8, 2), dev(8, 2), pp, {"min_score": 0.5})])
    with pytest.raises(ValueError, match="same place"):  # scores on the host
        api.SharedFocalBatch([(dev(8, 2), dev(8, 2), pp, {"scores": np.zeros(8)})])
