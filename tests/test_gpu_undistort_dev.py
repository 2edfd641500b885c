"""The un-distortion stage from device memory into device memory (pl_undistort_points_dev / pl_undistort_points_batch_dev):
every bit of the host entry point on the same values as doubles, NaN equal to NaN; nothing written beyond columns 0 and 1 of the
n destination rows; in place; the grouped form against its single calls; and the config-3 pipeline - undistort on the device,
estimate from the output arrays - against the all-host path."""
import ctypes as C
import json

import numpy as np
import pytest

import oracle_lib as O
from device_arrays import column_view, on_gpu, row_view
from device_results import bits, download, sentinel_array
from golden import make_golden_cameras as GC
from golden import make_golden_fisheye as GF
from poselib_amd import _lib as L
from poselib_amd import api, synth
from test_gpu_undistort import OPENCV, UNDISTORT_CAMERAS, _hostile_pixels, _pinhole_pixels

pytestmark = pytest.mark.gpu

SENTINEL = -12345.678
SIZES = [0, 1, 255, 256, 257, 1000]


def _cameras():
    """the eight models pl_undistort_points takes, with the parameters of the existing camera tests' fixtures"""
    cams = {"OPENCV": UNDISTORT_CAMERAS[0], "PINHOLE": UNDISTORT_CAMERAS[2],
            "SIMPLE_PINHOLE": {"model": "SIMPLE_PINHOLE", "width": 1280, "height": 720, "params": [900.0, 640.5, 360.25]}}
    json.load(open(GC.PATH)), json.load(open(GF.PATH))  # (the fixtures the cameras below were recorded with)
    for model in sorted(GC.MODELS):
        cams[model] = GC.named(GC.unproject_inputs(model)["disc"][0])
    for model in sorted(GF.MODELS):
        cams[model] = GF.named(GF.unproject_inputs(model)["disc"][0])
    assert len(cams) == 8
    return cams


CAMERAS = _cameras()
_PIXELS = {}


def pixels(model, n):
    """_hostile_pixels of the camera, the NaN / inf rows first so that every cut holds some, cut to n"""
    if model not in _PIXELS:
        cam = dict(CAMERAS[model])
        if len(cam["params"]) < 4 or model in ("SIMPLE_RADIAL", "RADIAL", "SIMPLE_RADIAL_FISHEYE", "RADIAL_FISHEYE"):
            cam = dict(cam, params=[cam["params"][0]] + list(cam["params"]))  # (f, cx, cy, ...: the helper reads params[2:4])
        pix = _hostile_pixels(cam)
        bad = ~np.isfinite(pix).all(axis=1)
        assert bad.sum() == 12
        pix = np.r_[pix[bad], pix[~bad]]
        pix.setflags(write=False)
        _PIXELS[model] = pix
    return _PIXELS[model][:n]


_HOST = {}


def host_result(gpu, model, values):
    """pl_undistort_points on the values as doubles, once per (model, input)"""
    key = (model, values.shape[0], values.tobytes()[:64], hash(values.tobytes()))
    if key not in _HOST:
        _HOST[key] = gpu.undistort_points(CAMERAS[model], values)
        _HOST[key].setflags(write=False)
    return _HOST[key]


def same_bits(got, want):
    assert got.shape == want.shape
    assert ((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))).all()


SOURCES = {
    "fp64": lambda x: on_gpu(x),
    "fp32": lambda x: on_gpu(x, np.float32),
    "fp32 column view": lambda x: column_view(x.astype(np.float32), np.float32),
    "fp64 column view": lambda x: column_view(x, np.float64),
    "fp32 row view": lambda x: row_view(x.astype(np.float32), np.float32),
    "fp64 row view": lambda x: row_view(x, np.float64),
}


def widened(x, source):
    with np.errstate(over="ignore"):
        return x.astype(np.float32).astype(np.float64) if source.startswith("fp32") else x


@pytest.mark.parametrize("model", sorted(CAMERAS))
def test_device_to_device_equals_the_host_call_bit_for_bit(gpu, model):
    for n in SIZES:
        x = pixels(model, n)
        for source in sorted(SOURCES):
            src = SOURCES[source](x) if n else on_gpu(np.zeros((0, 2)))
            want = host_result(gpu, model, widened(x, source))
            out = sentinel_array((n + 1, 2), np.float64, SENTINEL)
            dst = out[:n]
            assert gpu.undistort_points(CAMERAS[model], src, out=dst) is dst
            back = download(out)
            same_bits(back[:n], want)
            assert (back[n:] == SENTINEL).all(), (model, n, source)  # the row after the last
            if n >= 12:
                assert np.isnan(back[:12]).any()


@pytest.mark.parametrize("model", ["OPENCV", "RADIAL_FISHEYE", "SIMPLE_RADIAL"])
def test_a_strided_destination_keeps_what_lies_around_it(gpu, model):
    for n in SIZES:
        x = pixels(model, n)
        want = host_result(gpu, model, x)
        block = sentinel_array((n + 1, 4), np.float64, SENTINEL)
        gpu.undistort_points(CAMERAS[model], on_gpu(x) if n else on_gpu(np.zeros((0, 2))), out=block[:n, 1:3])
        back = download(block)
        same_bits(back[:n, 1:3], want)
        assert (back[:, 0] == SENTINEL).all() and (back[:, 3] == SENTINEL).all() and (back[n] == SENTINEL).all(), (model, n)


@pytest.mark.parametrize("model", ["OPENCV", "OPENCV_FISHEYE"])
def test_in_place(gpu, model):
    for n in SIZES[1:]:
        x = pixels(model, n)
        want = host_result(gpu, model, x)
        buf = on_gpu(np.array(x))
        assert gpu.undistort_points(CAMERAS[model], buf, out=buf) is buf
        same_bits(download(buf), want)
        # ... and as columns 0:2 of a wider block, whose other columns stay
        wide = np.full((n, 4), SENTINEL)
        wide[:, :2] = x
        block = on_gpu(wide)
        gpu.undistort_points(CAMERAS[model], block[:, :2], out=block[:, :2])
        back = download(block)
        same_bits(back[:, :2], want)
        assert (back[:, 2:] == SENTINEL).all()


def test_the_group_form_equals_its_single_calls_and_a_bad_member_fails_alone(gpu):
    lib = L.lib()
    sizes = [0, 1, 256, 257, 1000]
    models = ["OPENCV", "RADIAL_FISHEYE", "SIMPLE_RADIAL", "OPENCV", "RADIAL_FISHEYE"]
    makers = [SOURCES["fp64"], SOURCES["fp32"], SOURCES["fp32 column view"], SOURCES["fp64 row view"], SOURCES["fp32 row view"]]
    names = ["fp64", "fp32", "fp32 column view", "fp64 row view", "fp32 row view"]
    host_dst = np.full((256, 2), SENTINEL)  # member 2 writes to HOST memory: refused, nothing is written
    items = (L.UndistortItemDev * 5)()
    keep, blocks, wants = [], [], []
    for k, (n, model, make, name) in enumerate(zip(sizes, models, makers, names)):
        x = pixels(model, n)
        src = make(x) if n else on_gpu(np.zeros((0, 2)))
        block = sentinel_array((n + 1, 4), np.float64, SENTINEL)
        cam = gpu.Camera(CAMERAS[model]["model"], CAMERAS[model]["params"])._c()
        sd, rows, owner = api._device_points(src, 2)
        assert rows == n
        od, _ = api._device_points_out(block[:n, 1:3], n)
        if k == 2:
            od = L.DevicePointsOut(host_dst.ctypes.data, 2, L.PL_F64, 2)
        items[k].camera = C.pointer(cam)
        items[k].points2D, items[k].n, items[k].out = sd, n, od
        items[k].status = 99
        keep.append((cam, owner, src))
        blocks.append(block)
        wants.append(host_result(gpu, model, widened(x, name)))
    rc = lib.pl_undistort_points_batch_dev(items, 5)
    msg = lib.pl_last_error().decode()
    assert rc == L.PL_ERR_INVALID and "item 2:" in msg and "destination" in msg and "host" in msg, msg
    assert [it.status for it in items] == [0, 0, L.PL_ERR_INVALID, 0, 0]
    assert (host_dst == SENTINEL).all()
    for k, n in enumerate(sizes):
        back = download(blocks[k])
        if k == 2:
            assert (back == SENTINEL).all()
            continue
        same_bits(back[:n, 1:3], wants[k])
        assert (back[:, 0] == SENTINEL).all() and (back[:, 3] == SENTINEL).all() and (back[n] == SENTINEL).all()
    # the Python form: the same five members, all good, outputs returned in order
    outs = gpu.undistort_points_batch([(CAMERAS[m], keep[k][2], blocks[k][:sizes[k], 1:3]) for k, m in enumerate(models)])
    for k, n in enumerate(sizes):
        assert outs[k].shape == (n, 2)
        same_bits(download(blocks[k])[:n, 1:3], wants[k])


def test_a_destination_the_allocation_does_not_hold_is_refused(gpu):
    x = pixels("OPENCV", 257)
    block = sentinel_array((257, 4), np.float64, SENTINEL)
    short = block[:, 3:]  # (257, 1) columns: as an (n, 2) destination its last row would end 8 bytes beyond the allocation
    od = L.DevicePointsOut(short.data_ptr, 4, L.PL_F64, 2)
    sd, n, owner = api._device_points(on_gpu(x), 2)
    cam = gpu.Camera("OPENCV", CAMERAS["OPENCV"]["params"])._c()
    assert L.lib().pl_undistort_points_dev(C.byref(cam), C.byref(sd), n, C.byref(od)) == L.PL_ERR_INVALID
    assert "destination" in L.lib().pl_last_error().decode() and "beyond the allocation" in L.lib().pl_last_error().decode()
    assert (download(block) == SENTINEL).all()


def test_the_pipeline_on_device_arrays_equals_the_all_host_path(gpu):
    """a 300-correspondence OPENCV-distorted homography scene (generated as test_undistort_stage_in_front_of_the_two_view_estimators
    does): un-distorted on the device into columns of one (n, 4) block, estimated from those columns - model, mask and stats of the
    all-host path, bit for bit"""
    n = 300
    d = synth.homography_scene(n, 0.3, 1003)
    pin = {"model": "PINHOLE", "params": [1000.0, 1000.0, 500.0, 500.0]}
    x1d = synth.opencv_distort_pixels(_pinhole_pixels(OPENCV, O.unproject(pin, d["x1"])), OPENCV["params"])
    x2d = synth.opencv_distort_pixels(_pinhole_pixels(OPENCV, O.unproject(pin, d["x2"])), OPENCV["params"])
    opt = {"ransac": {"seed": 2}}
    u1, u2 = gpu.undistort_points(OPENCV, x1d), gpu.undistort_points(OPENCV, x2d)
    want_H, want = gpu.estimate_homography(u1, u2, opt)
    matches = on_gpu(np.c_[x1d, x2d])  # the matcher's (n, 4) block of distorted pixels ...
    clean = sentinel_array((n, 4), np.float64, SENTINEL)  # ... and one for the un-distorted ones
    o1, o2 = gpu.undistort_points_batch([(OPENCV, matches[:, :2], clean[:, :2]), (OPENCV, matches[:, 2:], clean[:, 2:])])
    got_H, got = gpu.estimate_homography(o1, o2, opt)
    assert got_H.tobytes() == want_H.tobytes()
    for k in ("refinements", "iterations", "num_inliers", "inlier_ratio", "model_score", "hypotheses", "inliers"):
        assert got[k] == want[k], k
    # 70 % of the rows are true inliers and the planar scene's default threshold keeps about two thirds of those (the standard of
    # tests/test_gpu_ranked_points.py): "solved" is more than 0.3 n, far above what a wrong model collects
    assert want["num_inliers"] > 0.3 * n
    same_bits(download(clean), np.c_[u1, u2])
