"""pl_estimate_batch_dev, the part that needs no device: the entry point and its record are declared, exported and bound; an
item is rejected before the device is touched, with its index in the message; the Python Batch turns device arrays into
pl_batch_item_dev records and refuses what a device call does not take.  No compute calls are made here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import poselib_amd
from poselib_amd import _lib as L
from poselib_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["pl_estimate_batch_dev", "pl_debug_point_stats_group_dev"]
FAR = 0x7F0000001000  # an address nothing dereferences


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
    assert "pl_batch_item_dev" in text
    # new symbols, no record changed: the layout version stays
    assert re.search(r"#define\s+PL_ABI_VERSION\s+5\b", text) and lib.pl_abi_version() == 5 and L.ABI_VERSION == 5


def test_batch_item_dev_layout():
    """pl_batch_item with the two pointers replaced by two 24-byte descriptors, by value; everything behind them moves by 32 bytes"""
    D, H = L.BatchItemDev, L.BatchItem
    assert C.sizeof(L.DevicePoints) == 24
    assert (D.kind.offset, D.status.offset, D.a.offset, D.b.offset, D.n.offset) == (0, 4, 8, 32, 56)
    assert D.a.size == 24 and D.b.size == 24
    for name in ("n", "opt", "camera1", "camera2", "model", "inliers", "stats"):
        assert getattr(D, name).offset == getattr(H, name).offset + 32, name
    assert C.sizeof(D) == C.sizeof(H) + 32 == 112


def _desc(data=FAR, row_stride=2, dtype=L.PL_F64, cols=2):
    return L.DevicePoints(data, row_stride, dtype, cols)


class _Items:
    """`count` plausible fundamental-matrix items (descriptors of addresses nothing reads), outputs kept alive"""

    def __init__(self, count, kind=2, n=100):
        self.items = (L.BatchItemDev * count)()
        self.keep = []
        for it in self.items:
            o = L.RobustOptions()
            L.lib().pl_default_robust_options(C.byref(o), kind if kind < 4 else (1 if kind == 4 else 5))
            model, st, inl = np.zeros(9), L.RansacStats(), np.zeros(n, dtype=np.uint8)
            cam = api.Camera("SIMPLE_PINHOLE", [1000.0, 500.0, 500.0])._c()
            it.kind, it.n = kind, n
            it.a, it.b = _desc(), _desc(cols=3, row_stride=3) if kind in (0, 5) else _desc()
            it.opt = C.pointer(o)
            it.camera1 = C.pointer(cam) if kind in (0, 1, 4) else None
            it.camera2 = C.pointer(cam) if kind == 1 else None
            it.model, it.inliers, it.stats = model.ctypes.data, inl.ctypes.data, C.pointer(st)
            self.keep.append((o, model, st, inl, cam))

    def run(self):
        return L.lib().pl_estimate_batch_dev(self.items, len(self.items), 4)


BAD = {
    "row_stride below cols": dict(row_stride=1),
    "unknown dtype": dict(dtype=2),
    "misaligned fp64": dict(data=FAR + 4),
}


@pytest.mark.skipif(poselib_amd.device_count() > 0, reason="GPU present")
@pytest.mark.parametrize("case", sorted(BAD))
@pytest.mark.parametrize("k", [0, 3, 6])
def test_a_bad_descriptor_is_named_by_its_item_before_the_device(case, k):
    b = _Items(7)
    b.items[k].b = _desc(**BAD[case])
    assert b.run() == L.PL_ERR_INVALID
    msg = L.lib().pl_last_error().decode()
    assert f"item {k}:" in msg and "device points" in msg, msg
    assert b.items[k].status == L.PL_ERR_INVALID
    assert all(b.items[i].status == L.PL_ERR_NO_DEVICE for i in range(7) if i != k)  # (the others would have run)


@pytest.mark.skipif(poselib_amd.device_count() > 0, reason="GPU present")
def test_a_plausible_batch_needs_the_device():
    b = _Items(5)
    assert b.run() == L.PL_ERR_NO_DEVICE
    assert L.lib().pl_estimate_batch_dev(None, 0, 4) == L.PL_OK  # (nothing to do)
    assert L.lib().pl_estimate_batch_dev(None, 3, 4) == L.PL_ERR_INVALID


@pytest.mark.skipif(poselib_amd.device_count() > 0, reason="GPU present")
def test_focal_and_radial_items_are_unsupported():
    for kind in (4, 5):
        b = _Items(3, kind=kind)
        assert b.run() == L.PL_ERR_UNSUPPORTED, kind
        assert "item 0:" in L.lib().pl_last_error().decode()
        assert [it.status for it in b.items] == [L.PL_ERR_UNSUPPORTED] * 3
    b = _Items(3, kind=0)
    b.keep[1][0].estimate_focal_length = 1
    assert b.run() == L.PL_ERR_UNSUPPORTED
    msg = L.lib().pl_last_error().decode()
    assert "item 1:" in msg and "estimate_focal_length" in msg, msg
    assert [it.status for it in b.items] == [L.PL_ERR_NO_DEVICE, L.PL_ERR_UNSUPPORTED, L.PL_ERR_NO_DEVICE]
    b = _Items(2)
    b.items[1].kind = 9
    assert b.run() == L.PL_ERR_INVALID and "item 1:" in L.lib().pl_last_error().decode()


class FakeDeviceArray:
    """__cuda_array_interface__ over a numpy buffer, whose address stands in for a device address; nothing dereferences it"""

    def __init__(self, array):
        self.array = array

    @property
    def __cuda_array_interface__(self):
        a = self.array
        return {"shape": a.shape, "typestr": a.dtype.str, "data": (a.__array_interface__["data"][0], False),
                "strides": None if a.flags.c_contiguous else tuple(a.strides), "version": 3}


def test_batch_builds_device_items_from_views_of_one_tensor():
    """the views of a padded (pairs, N, 4) float32 tensor: pointer, stride and dtype of every item's two descriptors"""
    t = np.zeros((3, 50, 4), dtype=np.float32)
    base = t.__array_interface__["data"][0]
    problems = [("hom", FakeDeviceArray(t[i, :, :2]), FakeDeviceArray(t[i, :, 2:]), {"ransac": {"seed": i}}) for i in range(3)]
    b = api.Batch(problems)
    assert b.on_device and isinstance(b.items[0], L.BatchItemDev) and len(b.items) == 3
    for i, it in enumerate(b.items):
        assert (it.kind, it.n) == (api.KIND_HOM, 50)
        assert (it.a.data, it.a.row_stride, it.a.dtype, it.a.cols) == (base + i * 50 * 16, 4, L.PL_F32, 2)
        assert (it.b.data, it.b.row_stride, it.b.dtype, it.b.cols) == (base + i * 50 * 16 + 8, 4, L.PL_F32, 2)
        assert it.opt.contents.ransac.seed == i and it.model and it.inliers
    # absolute pose: 2 and 3 columns, fp64, contiguous; the camera travels as for a host batch
    p2, p3 = np.zeros((20, 2)), np.zeros((20, 3))
    b = api.Batch([("abs", FakeDeviceArray(p2), FakeDeviceArray(p3), {"model": "SIMPLE_PINHOLE", "params": [800.0, 320.0, 240.0]}, None)])
    it = b.items[0]
    assert (it.a.data, it.a.row_stride, it.a.dtype, it.a.cols) == (p2.ctypes.data, 2, L.PL_F64, 2)
    assert (it.b.data, it.b.row_stride, it.b.dtype, it.b.cols) == (p3.ctypes.data, 3, L.PL_F64, 3)
    assert it.camera1.contents.params[0] == 800.0 and it.n == 20
    # host arrays: today's records
    b = api.Batch([("hom", np.zeros((8, 2)), np.zeros((8, 2)), None)])
    assert not b.on_device and isinstance(b.items[0], L.BatchItem)


def test_what_a_device_batch_refuses():
    dev = lambda *shape: FakeDeviceArray(np.zeros(shape))  # noqa: E731
    host = np.zeros((8, 2))
    with pytest.raises(ValueError, match="mixed"):  # host and device problems
        api.Batch([("hom", dev(8, 2), dev(8, 2), None), ("hom", host, host, None)])
    with pytest.raises(ValueError):  # ... and within one problem
        api.Batch([("hom", dev(8, 2), host, None)])
    with pytest.raises(ValueError, match="devices="):
        api.estimate_batch([("hom", dev(8, 2), dev(8, 2), None)], devices=[0])
    with pytest.raises(ValueError, match="devices="):
        api.Batch([("hom", dev(8, 2), dev(8, 2), None)]).run(devices="all")
    with pytest.raises(ValueError, match="shared_focal"):
        api.Batch([("shared_focal", dev(8, 2), dev(8, 2), (0.0, 0.0), None)])
    with pytest.raises(ValueError, match="radial1d"):
        api.Batch([("radial1d", dev(8, 2), dev(8, 3), None)])
    with pytest.raises(ValueError):  # sets of different length
        api.Batch([("hom", dev(8, 2), dev(9, 2), None)])
