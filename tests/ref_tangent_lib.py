"""ctypes access to the reference's tangent-Sampson relative-pose path through tests/ref_tangent/ref_tangent.cc - a small C
interface of our own, compiled against the reference's headers where they lie and linked to oracle/_ref/libposelib_ref.so
(tests/ref_lib.py builds that).  The driver is built into a temporary directory that lives as long as the process: nothing
compiled is kept, nothing is written under oracle/.  Test infrastructure only."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

import ref_lib

_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref_tangent", "ref_tangent.cc")
_ORACLE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle")
_lib = None


def available():
    return os.path.isdir(os.path.join(ref_lib.REFERENCE_ROOT, "PoseLib")) and ref_lib.available()


def lib():
    global _lib
    if _lib is None:
        ref_so = ref_lib.build()
        tmp = tempfile.mkdtemp(prefix="ref_tangent_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        out = os.path.join(tmp, "libref_tangent.so")
        # the flags of oracle/Makefile.ref: the headers' inline arithmetic compiles as in the reference build
        subprocess.check_call(["g++", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-w", "-shared", "-I", os.path.join(_ORACLE, "eigen_shim"),
                               "-I", ref_lib.REFERENCE_ROOT, "-o", out, _SRC, ref_so, "-Wl,-rpath," + os.path.dirname(ref_so)])
        L = C.CDLL(out)
        L.rt_focal.restype = C.c_double
        L.rt_score.restype = C.c_double
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a if shape is None else a.reshape(shape)


def _cam(cam):
    """(model id, parameter array, count) of a camera dict {"model": id, "params": [...]}; None: the identity camera"""
    if cam is None:
        return -1, np.zeros(1), 0
    par = _f64(cam["params"])
    return int(cam["model"]), (par if par.size else np.zeros(1)), int(par.size)


def focal(cam):
    m, par, k = _cam(cam)
    return float(lib().rt_focal(m, _p(par), k))


def rescale(cam, scale):
    """Camera::rescale: the camera dict with focal and principal-point parameters multiplied by scale"""
    if cam is None:
        return None
    m, par, k = _cam(cam)
    out = np.zeros(max(k, 1))
    lib().rt_rescale(m, _p(par), k, C.c_double(scale), _p(out))
    return dict(cam, params=[float(v) for v in out[:k]])


def unproject_with_jac(cam, pix):
    """d (n, 3), M (n, 6: 3x2 row-major), det(J J^T) (n,) of Camera::unproject_with_jac"""
    pix = _f64(pix, (-1, 2))
    n = pix.shape[0]
    m, par, k = _cam(cam)
    d, M, det = np.zeros((n, 3)), np.zeros((n, 6)), np.zeros(n)
    lib().rt_unproject_with_jac(m, _p(par), k, _p(pix), C.c_uint32(n), _p(d), _p(M), _p(det))
    return d, M, det


def score(pose, d1, d2, M1, M2, max_error):
    """(score, count, mask) of compute_tangent_sampson_msac_score / get_tangent_sampson_inliers"""
    d1, d2, M1, M2, pose = _f64(d1), _f64(d2), _f64(M1), _f64(M2), _f64(pose)
    n = d1.shape[0]
    cnt, mcnt = C.c_uint64(0), C.c_uint64(0)
    mask = np.zeros(max(n, 1), dtype=np.uint8)
    s = lib().rt_score(_p(pose), _p(d1), _p(d2), _p(M1), _p(M2), C.c_uint32(n), C.c_double(max_error * max_error), C.byref(cnt), _p(mask),
                       C.byref(mcnt))
    assert mcnt.value == cnt.value
    return float(s), int(cnt.value), mask[:n].astype(bool)


LOSS = {"TRIVIAL": 0, "TRUNCATED": 1, "HUBER": 2, "CAUCHY": 3}


def refine(pose, d1, d2, M1, M2, loss_type, loss_scale, max_iterations):
    """(pose, iterations, initial cost, cost) of refine_relpose(d1, d2, M1, M2, &pose, opt)"""
    d1, d2, M1, M2 = _f64(d1), _f64(d2), _f64(M1), _f64(M2)
    p = _f64(pose).copy()
    out = np.zeros(3)
    lib().rt_refine(_p(d1), _p(d2), _p(M1), _p(M2), C.c_uint32(d1.shape[0]), _p(p), LOSS[loss_type], C.c_double(loss_scale),
                    C.c_uint64(max_iterations), _p(out))
    return p, int(out[0]), float(out[1]), float(out[2])


def estimate_relative_pose(x1, x2, cam1, cam2, opt, initial_pose=None):
    """estimate_relative_pose(x1, x2, camera1, camera2, opt, &pose, &inliers) -> (pose (7,), mask, stats dict).  opt: max_error,
    tangent_sampson, ransac {seed, max_iterations, min_iterations, success_prob, progressive_sampling, score_initial_model}, bundle
    {loss_type, loss_scale, max_iterations} - every other field at the reference's default"""
    x1, x2 = _f64(x1, (-1, 2)), _f64(x2, (-1, 2))
    n = x1.shape[0]
    r, b = opt.get("ransac", {}), opt.get("bundle", {})
    unknown = (set(opt) - {"max_error", "tangent_sampson", "ransac", "bundle"}) | \
        (set(r) - {"seed", "max_iterations", "min_iterations", "success_prob", "progressive_sampling", "score_initial_model"}) | \
        (set(b) - {"loss_type", "loss_scale", "max_iterations"})
    assert not unknown, unknown
    iopt = np.array([r.get("max_iterations", 100000), r.get("min_iterations", 1000), r.get("seed", 0), int(r.get("progressive_sampling", False)),
                     int(r.get("score_initial_model", initial_pose is not None)), int(opt.get("tangent_sampson", False)),
                     LOSS[b.get("loss_type", "CAUCHY")], b.get("max_iterations", 100)], dtype=np.uint64)
    dopt = np.array([opt.get("max_error", 1.0), r.get("success_prob", 0.9999), b.get("loss_scale", 1.0)], dtype=np.float64)
    m1, p1, k1 = _cam(cam1)
    m2, p2, k2 = _cam(cam2)
    pose = _f64([1, 0, 0, 0, 0, 0, 0] if initial_pose is None else initial_pose).copy()
    mask = np.zeros(max(n, 1), dtype=np.uint8)
    st = np.zeros(5)
    lib().rt_estimate(_p(x1), _p(x2), C.c_uint32(n), m1, _p(p1), k1, m2, _p(p2), k2, _p(iopt), _p(dopt), _p(pose), _p(mask), _p(st))
    stats = {"refinements": int(st[0]), "iterations": int(st[1]), "num_inliers": int(st[2]), "inlier_ratio": float(st[3]),
             "model_score": float(st[4])}
    return pose, mask[:n].astype(bool), stats
