"""Python surface mirroring the reference's `poselib` module for the accelerated path.

Signatures, option-dict keys and return shapes follow the pybind11 module of PoseLib 3.0.0:
    estimate_absolute_pose(points2D, points3D, camera, opt={}, initial_pose=None) -> (Image, info)
        pybind/bindings/estimators/absolute_pose.cc:15-47, 317-330
    estimate_relative_pose(points2D_1, points2D_2, camera1, camera2, opt={}, initial_pose=None) -> (CameraPose, info)
        pybind/bindings/estimators/relative_pose.cc:15-52, 405-420
    estimate_fundamental(points2D_1, points2D_2, opt={}, initial_F=None) -> (3x3 ndarray, info)   (same file :221-243)
    estimate_homography(points2D_1, points2D_2, opt={}, initial_H=None) -> (3x3 ndarray, info)
        pybind/bindings/estimators/homography.cc:15-38, 75-77
    p3p / relpose_5pt / essential_matrix_5pt / relpose_7pt / homography_4pt   pybind/bindings/solvers.cc:305-365
Option dicts: nested 'ransac' / 'bundle' plus 'max_error', 'real_focal_check' (pybind/helpers.h:31-173);
`info` holds the RansacStats fields and 'inliers' as list[bool] (helpers.h:247-253, 266-272).
Passing an initial model sets ransac.score_initial_model (absolute_pose.cc(pybind):24-27).
All numerical work happens in the HIP library; this file only marshals numpy arrays through the C-ABI.
"""
from __future__ import annotations

import ctypes as C
import math
import sys
import threading

import numpy as np

from . import _lib as L

LAMBDA_UPDATES = {"NIELSEN": 0, "FIXED_FACTOR": 1}
DAMPINGS = {"LEVENBERG": 0, "MARQUARDT": 1}
LOSS_TYPES = {"TRIVIAL": 0, "TRUNCATED": 1, "HUBER": 2, "CAUCHY": 3, "TRUNCATED_CAUCHY": 4, "TRUNCATED_LE_ZACH": 5}
CAMERA_MODEL_IDS = {"NULL": -1, "SIMPLE_PINHOLE": 0, "PINHOLE": 1, "SIMPLE_RADIAL": 2, "RADIAL": 3, "OPENCV": 4,
                    "OPENCV_FISHEYE": 5, "SIMPLE_RADIAL_FISHEYE": 8, "RADIAL_FISHEYE": 9}
_CAMERA_NAMES = {v: k for k, v in CAMERA_MODEL_IDS.items()}
KIND_ABS, KIND_REL, KIND_FUND, KIND_HOM = 0, 1, 2, 3
KIND_SHARED_FOCAL = 4  # pl_batch_item only: estimate_shared_focal_relative_pose
KIND_RAD1D = 5  # absolute pose of a 1D-radial camera (centred pixels, no intrinsics)
_POSE_KINDS = (KIND_ABS, KIND_REL, KIND_RAD1D)  # problem kinds whose model is a CameraPose


# ------------------------------------------------------------------------------------------ types
class CameraPose:
    """poselib.CameraPose: q (w,x,y,z), t  (pybind/bindings/types.cc:35-45)."""

    def __init__(self, q=None, t=None):
        self.q = np.array([1.0, 0.0, 0.0, 0.0]) if q is None else np.asarray(q, dtype=np.float64).copy()
        self.t = np.zeros(3) if t is None else np.asarray(t, dtype=np.float64).copy()

    @property
    def R(self):
        w, x, y, z = self.q
        return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                         [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                         [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])

    @property
    def Rt(self):
        return np.concatenate([self.R, self.t[:, None]], axis=1)

    def center(self):
        return -self.R.T @ self.t

    def __repr__(self):
        return f"CameraPose(q={self.q.tolist()}, t={self.t.tolist()})"


class Camera:
    """poselib.Camera subset (pybind/bindings/types.cc:68-113)."""

    def __init__(self, model="SIMPLE_PINHOLE", params=(), width=0, height=0):
        if isinstance(model, dict):
            d = model
            model, params = d["model"], d["params"]
            width, height = d.get("width", 0), d.get("height", 0)
        self.model_id = CAMERA_MODEL_IDS[model] if isinstance(model, str) else int(model)
        self.params = [float(p) for p in params]
        self.width, self.height = int(width), int(height)

    def model_name(self):
        return _CAMERA_NAMES[self.model_id]

    def focal(self):
        if not self.params:
            return 1.0
        if self.model_id in (0, 2, 3, 8, 9):
            return self.params[0]
        if self.model_id in (1, 4, 5):
            return 0.5 * self.params[0] + 0.5 * self.params[1]
        return 1.0

    def todict(self):
        return {"model": self.model_name(), "width": self.width, "height": self.height, "params": list(self.params)}

    def _c(self) -> L.Camera:
        c = L.Camera()
        c.model_id, c.width, c.height, c.num_params = self.model_id, self.width, self.height, len(self.params)
        for i, v in enumerate(self.params):
            c.params[i] = v
        return c


class Image:
    """poselib.Image {camera, pose} (pybind/bindings/types.cc:117-119)."""

    def __init__(self, pose=None, camera=None):
        self.pose = pose or CameraPose()
        self.camera = camera or Camera()


def RansacOptions():
    return {"max_iterations": 100000, "min_iterations": 1000, "dyn_num_trials_mult": 3.0, "success_prob": 0.9999,
            "seed": 0, "progressive_sampling": False, "max_prosac_iterations": 100000}


def BundleOptions():
    return {"max_iterations": 100, "loss_type": "CAUCHY", "loss_scale": 1.0, "gradient_tol": 1e-12, "step_tol": 1e-8,
            "relative_cost_tol": 1e-10, "initial_lambda": 1e-3, "min_lambda": 1e-10, "max_lambda": 1e10,
            "lambda_factor": 10.0, "lambda_update": "NIELSEN", "damping": "LEVENBERG", "verbose": False}


# ------------------------------------------------------------------------------------------ marshalling
_RANSAC_KEYS = {"max_iterations", "min_iterations", "dyn_num_trials_mult", "success_prob", "seed",
                "progressive_sampling", "max_prosac_iterations", "score_initial_model"}
_BUNDLE_KEYS = {"max_iterations", "loss_type", "loss_scale", "gradient_tol", "step_tol", "relative_cost_tol",
                "initial_lambda", "min_lambda", "max_lambda", "lambda_factor", "lambda_update", "damping", "verbose",
                "refine_focal_length", "refine_extra_params", "refine_principal_point"}
_TOP_KEYS = {"ransac", "bundle", "max_error", "real_focal_check", "tangent_sampson", "estimate_focal_length",
             "estimate_extra_params", "min_fov"}


def _warn_unknown(d, known, where):
    # the reference's pybind ignores unknown keys silently (helpers.h:21-29); say so instead
    extra = sorted(set(d) - known)
    if extra:
        import warnings

        warnings.warn(f"poselib_amd: unknown {where} option(s) {extra} ignored", stacklevel=4)


def _robust_options(opt, kind: int, score_initial: bool) -> L.RobustOptions:
    o = L.RobustOptions()
    L.lib().pl_default_robust_options(C.byref(o), kind)
    opt = opt or {}
    _warn_unknown(opt, _TOP_KEYS, "top-level")
    _warn_unknown(opt.get("ransac", {}), _RANSAC_KEYS, "'ransac'")
    _warn_unknown(opt.get("bundle", {}), _BUNDLE_KEYS, "'bundle'")
    r = opt.get("ransac", {})
    for k in ("max_iterations", "min_iterations", "seed", "max_prosac_iterations"):
        if k in r:
            setattr(o.ransac, k, int(r[k]))
    for k in ("dyn_num_trials_mult", "success_prob"):
        if k in r:
            setattr(o.ransac, k, float(r[k]))
    if "progressive_sampling" in r:
        o.ransac.progressive_sampling = int(bool(r["progressive_sampling"]))
    o.ransac.score_initial_model = int(score_initial)
    b = opt.get("bundle", {})
    if "max_iterations" in b:
        o.bundle.max_iterations = int(b["max_iterations"])
    for k in ("loss_scale", "gradient_tol", "step_tol", "relative_cost_tol", "initial_lambda", "min_lambda",
              "max_lambda", "lambda_factor"):
        if k in b:
            setattr(o.bundle, k, float(b[k]))
    # enumerations: case-insensitive names like the reference's pybind (helpers.h:54-92), or the integer value
    for key, table in (("loss_type", LOSS_TYPES), ("lambda_update", LAMBDA_UPDATES), ("damping", DAMPINGS)):
        if key in b:
            v = b[key]
            setattr(o.bundle, key, table[v.upper()] if isinstance(v, str) else int(v))
    for k in ("refine_focal_length", "refine_extra_params", "refine_principal_point"):
        if k in b:
            setattr(o.bundle, k, int(bool(b[k])))
    if "max_error" in opt:
        o.max_error = float(opt["max_error"])
    for k in ("real_focal_check", "tangent_sampson", "estimate_focal_length", "estimate_extra_params"):
        if k in opt:
            setattr(o, k, int(bool(opt[k])))
    if "min_fov" in opt:  # types.h:126; read by the focal-length estimator only (absolute_pose.h:78)
        o.min_fov = float(opt["min_fov"])
    return o


def _pts(a, dim):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != dim:
        raise ValueError(f"expected an (N, {dim}) array")
    return a


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- points that are already on the GPU: torch tensors, or any object with __cuda_array_interface__ (recognised by attribute,
# torch is never imported here).  They reach the library as pl_device_points descriptors - float32 or float64, rows any number of
# elements apart - and are read where they lie: nothing is copied to the host.
_tls = threading.local()  # .device: what set_device() selected on this thread (0 before the first call, like the library)
_TORCH_DTYPES = {"torch.float32": L.PL_F32, "torch.float64": L.PL_F64}
_TYPESTR_DTYPES = {"<f4": (L.PL_F32, 4), "<f8": (L.PL_F64, 8), "=f4": (L.PL_F32, 4), "=f8": (L.PL_F64, 8)}


def _selected_device() -> int:
    return getattr(_tls, "device", 0)


def _is_torch_tensor(a) -> bool:
    return hasattr(a, "is_cuda") and hasattr(a, "data_ptr") and hasattr(a, "stride")


def _on_device(a) -> bool:
    if _is_torch_tensor(a):
        return bool(a.is_cuda)  # (a CPU tensor goes the host way, through numpy)
    return not isinstance(a, np.ndarray) and hasattr(a, "__cuda_array_interface__")


def _device_points(a, dim, streams=None):
    """(pl_device_points descriptor, rows, the object that owns the memory) of a GPU tensor or __cuda_array_interface__ object.
    float32 / float64 only; a column stride other than 1 is made contiguous on the device (the object's own .contiguous());
    a torch tensor must live on the device this thread selected, and its current stream is synchronised - the library reads the
    memory on a stream of its own and takes none from the caller.  streams: a dict that collects {device: (torch, device)}
    instead - the caller synchronises every device once when all its descriptors are made (_sync_streams; Batch)."""
    if _is_torch_tensor(a):
        if a.dim() != 2 or a.shape[1] != dim:
            raise ValueError(f"expected an (N, {dim}) tensor")
        dtype = _TORCH_DTYPES.get(str(a.dtype))
        if dtype is None:
            raise ValueError(f"device points must be float32 or float64, not {a.dtype}")
        index = a.device.index
        torch = sys.modules.get(type(a).__module__.split(".")[0])
        if index is None and torch is not None:
            index = torch.cuda.current_device()
        if index != _selected_device():
            raise ValueError(f"the tensor lives on device {index}, this thread selected device {_selected_device()} (set_device)")
        n = int(a.shape[0])
        if n > 1 and (a.stride(1) != 1 or a.stride(0) < dim):
            a = a.contiguous()
        if torch is not None:
            if streams is None:
                torch.cuda.current_stream(a.device).synchronize()
            else:
                streams.setdefault(index, (torch, a.device))
        row = int(a.stride(0)) if n > 1 else dim
        return L.DevicePoints(a.data_ptr() if n else None, row, dtype, dim), n, a
    cai = a.__cuda_array_interface__
    shape = tuple(cai["shape"])
    if len(shape) != 2 or shape[1] != dim:
        raise ValueError(f"expected an (N, {dim}) array")
    if cai["typestr"] not in _TYPESTR_DTYPES:
        raise ValueError(f"device points must be float32 or float64, not typestr {cai['typestr']!r}")
    dtype, size = _TYPESTR_DTYPES[cai["typestr"]]
    n = int(shape[0])
    strides = cai.get("strides")
    if strides is None:
        row, col = dim, 1
    else:
        if strides[0] % size or strides[1] % size:
            raise ValueError("byte strides of the device array are no multiple of its element size")
        row, col = strides[0] // size, strides[1] // size
    if n > 1 and (col != 1 or row < dim):
        if not hasattr(a, "contiguous"):
            raise ValueError("device points need a column stride of 1 (and the object has no .contiguous() to make them so)")
        b = a.contiguous()
        bs = b.__cuda_array_interface__.get("strides")
        if bs is not None and tuple(bs) != (dim * size, size):
            raise ValueError(".contiguous() of the device array did not return a contiguous array")
        return _device_points(b, dim, streams)
    if n <= 1:
        row = dim
    return L.DevicePoints(int(cai["data"][0]) if n else None, int(row), dtype, dim), n, a


def _sync_streams(streams):
    for torch, device in streams.values():
        torch.cuda.current_stream(device).synchronize()


# ---- one confidence per row (a matcher's scores): which rows are correspondences, and in which order.  THE RULE
# (include/poselib_amd.h): row i is kept iff scores[i] >= min_score (a NaN never is; min_score defaults to -inf), kept rows go in
# descending score, equal scores (-0.0 == 0.0) in ascending row index.  Scores reorder and select; they do not switch PROSAC on -
# ransac.progressive_sampling does, as everywhere.
def _min_score(min_score) -> float:
    m = -math.inf if min_score is None else float(min_score)
    if m != m:
        raise ValueError("min_score is NaN")
    return m


def score_order(scores, min_score=None):
    """THE RULE in numpy, for scores in host memory: the rows that are used, in the order they are used.  float32 scores are
    widened (exactly) first, so a float32 array ranks like the same values as doubles - and like the device kernels."""
    s = np.asarray(scores)
    if s.ndim != 1 or s.dtype not in (np.float32, np.float64):
        raise ValueError("scores: expected a one-dimensional float32 or float64 array")
    s = s.astype(np.float64)
    keep = s >= _min_score(min_score)
    return np.flatnonzero(keep)[np.argsort(-s[keep], kind="stable")]


def _device_scores(scores, n, min_score, streams=None):
    """(pl_device_scores descriptor, the object that owns the memory) of a one-dimensional GPU tensor / __cuda_array_interface__
    object of n elements - a column view of a wider block keeps its stride.  Synchronisation as _device_points."""
    m = _min_score(min_score)
    if _is_torch_tensor(scores):
        if scores.dim() != 1:
            raise ValueError("scores: expected a one-dimensional tensor")
        dtype = _TORCH_DTYPES.get(str(scores.dtype))
        if dtype is None:
            raise ValueError(f"device scores must be float32 or float64, not {scores.dtype}")
        index = scores.device.index
        torch = sys.modules.get(type(scores).__module__.split(".")[0])
        if index is None and torch is not None:
            index = torch.cuda.current_device()
        if index != _selected_device():
            raise ValueError(f"the scores live on device {index}, this thread selected device {_selected_device()} (set_device)")
        rows = int(scores.shape[0])
        if rows > 1 and scores.stride(0) < 1:
            scores = scores.contiguous()
        if torch is not None:
            if streams is None:
                torch.cuda.current_stream(scores.device).synchronize()
            else:
                streams.setdefault(index, (torch, scores.device))
        stride, ptr = (int(scores.stride(0)) if rows > 1 else 1), (scores.data_ptr() if rows else None)
    else:
        cai = scores.__cuda_array_interface__
        shape = tuple(cai["shape"])
        if len(shape) != 1:
            raise ValueError("scores: expected a one-dimensional array")
        if cai["typestr"] not in _TYPESTR_DTYPES:
            raise ValueError(f"device scores must be float32 or float64, not typestr {cai['typestr']!r}")
        dtype, size = _TYPESTR_DTYPES[cai["typestr"]]
        rows = int(shape[0])
        strides = cai.get("strides")
        stride = 1
        if strides is not None and rows > 1:
            if strides[0] % size or strides[0] < size:
                raise ValueError("the byte stride of the device scores is no positive multiple of their element size")
            stride = strides[0] // size
        ptr = int(cai["data"][0]) if rows else None
    if rows != n:
        raise ValueError(f"{rows} scores for {n} correspondences")
    return L.DeviceScores(ptr, stride, dtype, 0, m), scores


def _device_mask(mask, n, streams=None):
    """(pl_device_mask descriptor, the object that owns the memory) of inliers_out=: a one-dimensional GPU tensor /
    __cuda_array_interface__ object of n one-byte elements (torch.bool, torch.uint8), strided allowed - the library writes one 0 / 1
    byte per row there.  Synchronisation as _device_points."""
    if _is_torch_tensor(mask):
        if not mask.is_cuda:
            raise ValueError("inliers_out= must be on the GPU")
        if str(mask.dtype) not in ("torch.bool", "torch.uint8"):
            raise ValueError(f"inliers_out= must be torch.bool or torch.uint8, not {mask.dtype}")
        if mask.dim() != 1 or int(mask.shape[0]) != n:
            raise ValueError(f"inliers_out=: expected {n} elements, got shape {tuple(mask.shape)}")
        index = mask.device.index
        torch = sys.modules.get(type(mask).__module__.split(".")[0])
        if index is None and torch is not None:
            index = torch.cuda.current_device()
        if index != _selected_device():
            raise ValueError(f"inliers_out= lives on device {index}, this thread selected device {_selected_device()} (set_device)")
        if n > 1 and mask.stride(0) < 1:
            raise ValueError("inliers_out= needs a positive stride")
        if torch is not None:
            if streams is None:
                torch.cuda.current_stream(mask.device).synchronize()
            else:
                streams.setdefault(index, (torch, mask.device))
        return L.DeviceMask(mask.data_ptr() if n else None, int(mask.stride(0)) if n > 1 else 1), mask
    if not _on_device(mask):
        raise ValueError("inliers_out= must be on the GPU")
    cai = mask.__cuda_array_interface__
    shape = tuple(cai["shape"])
    if cai["typestr"] not in ("|b1", "|u1"):
        raise ValueError(f"inliers_out= must hold one-byte bool / uint8 elements, not typestr {cai['typestr']!r}")
    if len(shape) != 1 or int(shape[0]) != n:
        raise ValueError(f"inliers_out=: expected {n} elements, got shape {shape}")
    if cai["data"][1]:
        raise ValueError("inliers_out= is read-only")
    strides = cai.get("strides")
    stride = 1
    if strides is not None and n > 1:
        if strides[0] < 1:
            raise ValueError("inliers_out= needs a positive stride")
        stride = int(strides[0])
    return L.DeviceMask(int(cai["data"][0]) if n else None, stride), mask


def _check_mask_args(on_device, inliers_out):
    if inliers_out is not None and not on_device:
        raise ValueError("inliers_out= goes with points on the GPU: host points return info['inliers'] as a list")


def _check_scores_args(on_device, scores, min_score):
    if scores is None:
        if min_score is not None:
            raise ValueError("min_score without scores")
        return
    if on_device != _on_device(scores):
        raise ValueError("points and scores must be in the same place: both on the GPU or both in host memory")


def _scored_host(call, a, b, scores, min_score):
    """scores in host memory: THE RULE in numpy, the plain call on a[order], b[order], the mask back in the caller's numbering"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    order = score_order(scores, min_score)
    if len(np.asarray(scores)) != a.shape[0]:
        raise ValueError(f"{len(np.asarray(scores))} scores for {a.shape[0]} correspondences")
    model, info = call(a[order], b[order])
    mask = np.zeros(a.shape[0], dtype=bool)
    mask[order] = info["inliers"]
    info["inliers"] = mask.tolist()
    info["n_used"] = int(len(order))
    return model, info


class _Points:
    """The two point sets of a call as the C-ABI takes them: host arrays (pointers to float64 data) or device descriptors."""

    def __init__(self, a, b, dim_a, dim_b):
        self.on_device = _on_device(a)
        if self.on_device != _on_device(b):
            raise ValueError("one point set is on the GPU and the other in host memory: pass both the same way")
        if self.on_device:
            da, self.n, keep_a = _device_points(a, dim_a)
            db, nb, keep_b = _device_points(b, dim_b)
            if nb != self.n:
                raise ValueError(f"the point sets differ in length ({self.n} and {nb})")
            self.keep = (da, db, keep_a, keep_b)
            self.a, self.b = C.byref(da), C.byref(db)
        else:
            a, b = _pts(a, dim_a), _pts(b, dim_b)
            self.n = a.shape[0]
            self.keep = (a, b)
            self.a, self.b = _ptr(a), _ptr(b)

    def fn(self, name):
        return getattr(L.lib(), name + "_dev" if self.on_device else name)


def _info(st: L.RansacStats, inliers, n_used=None):
    """inliers: the host mask (becomes a list of bool), or the caller's inliers_out= object, which is handed back as it is"""
    host = isinstance(inliers, np.ndarray)
    return {"n_used": len(inliers) if n_used is None else int(n_used),  # rows the estimator ran on (fewer than given: scores=)
            "refinements": st.refinements, "iterations": st.iterations, "num_inliers": st.num_inliers,
            "inlier_ratio": st.inlier_ratio, "model_score": st.model_score, "inliers": inliers.astype(bool).tolist() if host else inliers,
            # extras (not in the reference): metric numerator and device timing
            "hypotheses": st.hypotheses, "iterations_evaluated": st.iterations_evaluated, "seconds": st.seconds,
            "score_kernel_ms": st.score_kernel_ms, "score_kernel_launches": st.score_kernel_launches,
            "nan_hypotheses": st.nan_hypotheses}


def _cpose(p: CameraPose) -> L.CameraPose:
    c = L.CameraPose()
    for i in range(4):
        c.q[i] = p.q[i]
    for i in range(3):
        c.t[i] = p.t[i]
    return c


def _pypose(c: L.CameraPose) -> CameraPose:
    return CameraPose(np.array(c.q[:]), np.array(c.t[:]))


def _as_camera(cam) -> Camera:
    return cam if isinstance(cam, Camera) else Camera(cam)


# ------------------------------------------------------------------------------------------ estimators
def _run_scored(kind, pts, scores, min_score, o, c1, c2, model, inl, st, inliers_out=None):
    """pl_estimate_dev_scored: device points with device scores; with inliers_out= (and then with or without scores)
    pl_estimate_dev_masked: the mask stays on the device.  Returns n_used"""
    sd, keep = _device_scores(scores, pts.n, min_score) if scores is not None else (None, None)
    used = C.c_size_t(0)
    cams = (None if c1 is None else C.byref(c1), None if c2 is None else C.byref(c2))
    if inliers_out is not None:
        md, keep_mask = _device_mask(inliers_out, pts.n)
        L.check(L.lib().pl_estimate_dev_masked(kind, pts.a, pts.b, None if sd is None else C.byref(sd), C.c_size_t(pts.n), C.byref(o),
                                               cams[0], cams[1], model, C.byref(md), C.byref(st), C.byref(used)))
        del keep_mask
    else:
        L.check(L.lib().pl_estimate_dev_scored(kind, pts.a, pts.b, C.byref(sd), C.c_size_t(pts.n), C.byref(o), cams[0], cams[1], model,
                                               _ptr(inl), C.byref(st), C.byref(used)))
    del keep
    return int(used.value)


def estimate_absolute_pose(points2D, points3D, camera, opt=None, initial_pose=None, scores=None, min_score=None, inliers_out=None):
    """scores (one per row, where the points are) / min_score: the rows with score >= min_score are used, in descending score -
    see score_order; info["inliers"] keeps the caller's numbering, info["n_used"] is the number of rows used.
    inliers_out (points on the GPU only): a device array of n one-byte elements (torch.bool / torch.uint8, strided allowed) that
    receives the mask - it never comes down: info["inliers"] is that object and no list is built"""
    _check_scores_args(_on_device(points2D) or _on_device(points3D), scores, min_score)
    _check_mask_args(_on_device(points2D) or _on_device(points3D), inliers_out)
    if scores is not None and not _on_device(scores):
        return _scored_host(lambda a, b: estimate_absolute_pose(a, b, camera, opt, initial_pose), points2D, points3D, scores, min_score)
    pts = _Points(points2D, points3D, 2, 3)
    cam = _as_camera(camera)
    o = _robust_options(opt, KIND_ABS, initial_pose is not None)
    c = cam._c()
    pose = _cpose(initial_pose if initial_pose is not None else CameraPose())
    n = pts.n
    inl = np.zeros(max(n, 1), dtype=np.uint8)
    st = L.RansacStats()
    used = None
    if scores is not None or inliers_out is not None:
        used = _run_scored(KIND_ABS, pts, scores, min_score, o, c, None, C.cast(C.pointer(pose), C.c_void_p), inl, st, inliers_out)
        used = used if scores is not None else None
    else:
        L.check(pts.fn("pl_estimate_absolute_pose")(pts.a, pts.b, C.c_size_t(n), C.byref(o), C.byref(c), C.byref(pose),
                                                    _ptr(inl), C.byref(st)))
    out_cam = Camera(cam.model_id, list(c.params[: c.num_params]), cam.width, cam.height)
    return Image(_pypose(pose), out_cam), _info(st, inl[:n] if inliers_out is None else inliers_out, n if used is None else used)


def estimate_relative_pose(points2D_1, points2D_2, camera1, camera2, opt=None, initial_pose=None, scores=None, min_score=None,
                           inliers_out=None):
    _check_scores_args(_on_device(points2D_1) or _on_device(points2D_2), scores, min_score)
    _check_mask_args(_on_device(points2D_1) or _on_device(points2D_2), inliers_out)
    if scores is not None and not _on_device(scores):
        return _scored_host(lambda a, b: estimate_relative_pose(a, b, camera1, camera2, opt, initial_pose), points2D_1, points2D_2,
                            scores, min_score)
    pts = _Points(points2D_1, points2D_2, 2, 2)
    c1, c2 = _as_camera(camera1)._c(), _as_camera(camera2)._c()
    o = _robust_options(opt, KIND_REL, initial_pose is not None)
    pose = _cpose(initial_pose if initial_pose is not None else CameraPose())
    n = pts.n
    inl = np.zeros(max(n, 1), dtype=np.uint8)
    st = L.RansacStats()
    used = None
    if scores is not None or inliers_out is not None:
        used = _run_scored(KIND_REL, pts, scores, min_score, o, c1, c2, C.cast(C.pointer(pose), C.c_void_p), inl, st, inliers_out)
        used = used if scores is not None else None
    else:
        L.check(pts.fn("pl_estimate_relative_pose")(pts.a, pts.b, C.c_size_t(n), C.byref(c1), C.byref(c2), C.byref(o),
                                                    C.byref(pose), _ptr(inl), C.byref(st)))
    return _pypose(pose), _info(st, inl[:n] if inliers_out is None else inliers_out, n if used is None else used)


def _estimate_matrix(fn, kind, points2D_1, points2D_2, opt, initial, scores=None, min_score=None, inliers_out=None):
    _check_scores_args(_on_device(points2D_1) or _on_device(points2D_2), scores, min_score)
    _check_mask_args(_on_device(points2D_1) or _on_device(points2D_2), inliers_out)
    if scores is not None and not _on_device(scores):
        return _scored_host(lambda a, b: _estimate_matrix(fn, kind, a, b, opt, initial), points2D_1, points2D_2, scores, min_score)
    pts = _Points(points2D_1, points2D_2, 2, 2)
    o = _robust_options(opt, kind, initial is not None)
    M = np.ascontiguousarray((np.eye(3) if initial is None else np.asarray(initial, dtype=np.float64)).T.reshape(9))
    n = pts.n
    inl = np.zeros(max(n, 1), dtype=np.uint8)
    st = L.RansacStats()
    used = None
    if scores is not None or inliers_out is not None:
        used = _run_scored(kind, pts, scores, min_score, o, None, None, _ptr(M), inl, st, inliers_out)
        used = used if scores is not None else None
    else:
        L.check(pts.fn(fn)(pts.a, pts.b, C.c_size_t(n), C.byref(o), _ptr(M), _ptr(inl), C.byref(st)))
    return M.reshape(3, 3).T.copy(), _info(st, inl[:n] if inliers_out is None else inliers_out, n if used is None else used)


class _DevicePts:
    """One device point set of a Batch problem: its descriptor, its rows (.shape like an array) and the object that owns the memory"""

    def __init__(self, a, dim, streams):
        self.desc, n, self.owner = _device_points(a, dim, streams)
        self.shape = (n, dim)


class Batch:
    """An array of pl_batch_item descriptors (include/poselib_amd.h) marshalled once: `run()` is the C-ABI call
    pl_estimate_batch and nothing else (what bench_batch.py times), `results()` turns the outputs into the objects the
    single-problem functions return.

    The point sets of a problem may be GPU tensors or __cuda_array_interface__ objects instead of arrays (the views of a matcher's
    padded (pairs, N, 4) tensor): the items then are pl_batch_item_dev records and `run()` is pl_estimate_batch_dev - nothing is
    copied to the host.  A call is all-device or all-host; "shared_focal" and "radial1d" problems and `devices=` are host-only
    (shared-focal pairs on the GPU: SharedFocalBatch)."""

    def __init__(self, problems):
        kinds = {"abs": KIND_ABS, "rel": KIND_REL, "fund": KIND_FUND, "hom": KIND_HOM, "shared_focal": KIND_SHARED_FOCAL,
                 "radial1d": KIND_RAD1D}
        where = {_on_device(pr[1]) or _on_device(pr[2]) for pr in problems}
        if len(where) > 1:
            raise ValueError("host and device problems are mixed in one batch: a call is all-device or all-host")
        self.on_device = True in where
        if self.on_device:
            for pr in problems:
                if pr[0] in ("shared_focal", "radial1d"):
                    raise ValueError(f"a {pr[0]!r} problem is not served from device memory: pass host arrays" +
                                     (" (pairs on the GPU: SharedFocalBatch)" if pr[0] == "shared_focal" else ""))
                if _on_device(pr[1]) != _on_device(pr[2]):
                    raise ValueError("one point set is on the GPU and the other in host memory: pass both the same way")
        streams = {}

        # (device points: the descriptor, the rows and the owner travel as one object)
        pts = (lambda a, dim: _DevicePts(a, dim, streams)) if self.on_device else _pts

        self.items = ((L.BatchItemDev if self.on_device else L.BatchItem) * len(problems))()
        self.keep = []
        self.mask_out = []  # per problem: the caller's inliers_out= object or None
        # device items with scores: pl_estimate_batch_dev_scored (an entry without data is a plain item)
        self.scores = (L.DeviceScores * max(len(problems), 1))()
        self.n_used = (C.c_size_t * max(len(problems), 1))()
        self.scored = False
        # device items with "inliers_out": pl_estimate_batch_dev_masked (an entry without data keeps its host mask)
        self.masks = (L.DeviceMask * max(len(problems), 1))()
        self.masked = False
        for it, pr in zip(self.items, problems):
            kind = kinds[pr[0]]
            it.kind = kind
            # a warm start: the options dict may carry "initial_model" (a CameraPose for "abs" / "rel", a 3 x 3 matrix for "fund" /
            # "hom") - the initial_pose / initial_F / initial_H argument of the single-problem functions; it sets score_initial_model
            # ... and "scores" / "min_score": one confidence per row, where the points are (score_order has the rule)
            opt = dict(pr[-1] or {})
            init = opt.pop("initial_model", None)
            scores, min_score = opt.pop("scores", None), opt.pop("min_score", None)
            _check_scores_args(self.on_device, scores, min_score)
            # ... and "inliers_out": a device array of n one-byte elements that receives the mask (device points only)
            inliers_out = opt.pop("inliers_out", None)
            _check_mask_args(self.on_device, inliers_out)
            order, rows = None, None
            if scores is not None and not self.on_device:  # host points: the rule in numpy, the plain item on the ranked rows
                order = score_order(scores, min_score)
                rows = len(np.asarray(scores))
                pa, pb = np.asarray(pr[1], dtype=np.float64), np.asarray(pr[2], dtype=np.float64)
                if pa.shape[0] != rows or pb.shape[0] != rows:
                    raise ValueError(f"{rows} scores for {pa.shape[0]} and {pb.shape[0]} correspondences")
                pr = (pr[0], pa[order], pb[order]) + tuple(pr[3:])
            pr = tuple(pr[:-1]) + (opt,)
            if kind == KIND_ABS:
                _, a, b, cam, opt = pr
                a, b = pts(a, 2), pts(b, 3)
                cam = _as_camera(cam)
                c1, c2 = cam._c(), None
                model = _cpose(init if init is not None else CameraPose())
            elif kind == KIND_REL:
                _, a, b, cam1, cam2, opt = pr
                a, b = pts(a, 2), pts(b, 2)
                cam = None
                c1, c2 = _as_camera(cam1)._c(), _as_camera(cam2)._c()
                model = _cpose(init if init is not None else CameraPose())
            elif kind == KIND_RAD1D:  # ("radial1d", centred pixels, points3D, opt)
                _, a, b, opt = pr
                a, b = pts(a, 2), pts(b, 3)
                cam, c1, c2 = None, None, None
                model = _cpose(init if init is not None else CameraPose())
            elif kind == KIND_SHARED_FOCAL:
                _, a, b, pp, opt = pr
                a, b = pts(a, 2), pts(b, 2)
                cam = Camera("SIMPLE_PINHOLE", [1.0, float(pp[0]), float(pp[1])])
                c1, c2 = cam._c(), None
                model = _cpose(CameraPose())
            else:
                _, a, b, opt = pr
                a, b = pts(a, 2), pts(b, 2)
                cam, c1, c2 = None, None, None
                model = np.ascontiguousarray((np.eye(3) if init is None else np.asarray(init, dtype=np.float64)).T.reshape(9))
            o = _robust_options(opt, KIND_REL if kind == KIND_SHARED_FOCAL else kind, init is not None and kind != KIND_SHARED_FOCAL)
            n = a.shape[0]
            if b.shape[0] != n and self.on_device:
                raise ValueError(f"the point sets differ in length ({n} and {b.shape[0]})")
            inl = np.zeros(max(n, 1), dtype=np.uint8)
            st = L.RansacStats()
            if self.on_device:
                it.a, it.b, it.n = a.desc, b.desc, n
                if scores is not None:
                    self.scores[len(self.keep)], order = _device_scores(scores, n, min_score, streams)  # (order: keeps the owner)
                    self.scored = True
                if inliers_out is not None:
                    self.masks[len(self.keep)], inliers_out = _device_mask(inliers_out, n, streams)
                    self.masked = True
            else:
                it.a, it.b, it.n = _ptr(a), _ptr(b), n
            it.opt = C.pointer(o)
            it.camera1 = C.pointer(c1) if c1 is not None else None
            it.camera2 = C.pointer(c2) if c2 is not None else None
            it.model = C.cast(C.pointer(model), C.c_void_p) if kind in (KIND_ABS, KIND_REL, KIND_SHARED_FOCAL, KIND_RAD1D) else _ptr(model)
            it.inliers = _ptr(inl)
            it.stats = C.pointer(st)
            self.keep.append((kind, a, b, o, cam, c1, c2, model, inl, st, n, order, rows))
            self.mask_out.append(inliers_out)
        _sync_streams(streams)  # (once per device, not per tensor: the producers' work is complete before run())

    def run(self, max_in_flight=8, devices=None):
        """devices: None = the calling thread's device (pl_estimate_batch); a list of device indices, or "all", = the items
        round-robined over those devices from this one process (pl_estimate_batch_devices)"""
        if self.on_device:
            if devices is not None:
                raise ValueError("devices= with device points: the memory belongs to one device (set_device selects it)")
            if self.masked:
                L.check(L.lib().pl_estimate_batch_dev_masked(self.items, self.scores if self.scored else None, self.masks, self.n_used,
                                                             C.c_size_t(len(self.keep)), C.c_int(int(max_in_flight))))
                return
            if self.scored:
                L.check(L.lib().pl_estimate_batch_dev_scored(self.items, self.scores, self.n_used, C.c_size_t(len(self.keep)),
                                                             C.c_int(int(max_in_flight))))
                return
            L.check(L.lib().pl_estimate_batch_dev(self.items, C.c_size_t(len(self.keep)), C.c_int(int(max_in_flight))))
            return
        if devices is None:
            L.check(L.lib().pl_estimate_batch(self.items, C.c_size_t(len(self.keep)), C.c_int(int(max_in_flight))))
            return
        lst = [] if isinstance(devices, str) else [int(d) for d in devices]
        arr = (C.c_int * max(len(lst), 1))(*lst)
        L.check(L.lib().pl_estimate_batch_devices(self.items, C.c_size_t(len(self.keep)), arr if lst else None, C.c_int(len(lst)),
                                                  C.c_int(int(max_in_flight))))

    def stats(self):
        """(iterations, num_inliers, hypotheses) arrays without building the per-problem Python objects"""
        it = np.array([k[9].iterations for k in self.keep], dtype=np.int64)
        ni = np.array([k[9].num_inliers for k in self.keep], dtype=np.int64)
        hy = np.array([k[9].hypotheses for k in self.keep], dtype=np.int64)
        return it, ni, hy

    def results(self):
        out = []
        for i, (kind, a, b, o, cam, c1, c2, model, inl, st, n, order, rows) in enumerate(self.keep):
            if self.on_device:
                info = _info(st, inl[:n] if self.mask_out[i] is None else self.mask_out[i], self.n_used[i] if self.scored else n)
            elif rows is not None:  # host scores: the mask of the ranked rows back in the caller's numbering
                mask = np.zeros(rows, dtype=np.uint8)
                mask[order] = inl[:n]
                info = _info(st, mask, n)
            else:
                info = _info(st, inl[:n])
            if kind == KIND_ABS:
                out_cam = Camera(cam.model_id, list(c1.params[: c1.num_params]), cam.width, cam.height)
                out.append((Image(_pypose(model), out_cam), info))
            elif kind in (KIND_REL, KIND_RAD1D):
                out.append((_pypose(model), info))
            elif kind == KIND_SHARED_FOCAL:
                out.append((_shared_focal_pair(model, c1.params[0], (c1.params[1], c1.params[2])), info))
            else:
                out.append((model.reshape(3, 3).T.copy(), info))
        return out


def last_batch_report():
    """What this thread's last batch call did with its items (include/poselib_amd.h pl_batch_report): items in lock-step groups run
    at the advertised rate, `solo` and `fallback` items one at a time."""
    r = L.BatchReport()
    L.lib().pl_last_batch_report(C.byref(r))
    return {k: int(getattr(r, k)) for k in ("items", "grouped", "focal_grouped", "solo", "fallback")}


def estimate_batch(problems, max_in_flight=8, devices=None):
    """Many independent problems in one call (include/poselib_amd.h pl_estimate_batch; BASELINE config 4).

    problems: list of tuples, the arguments of the single-problem functions prefixed by the kind:
        ("abs", points2D, points3D, camera, opt)            -> (Image, info)
        ("rel", points2D_1, points2D_2, camera1, camera2, opt) -> (CameraPose, info)
        ("fund", points2D_1, points2D_2, opt) / ("hom", points2D_1, points2D_2, opt) -> (3x3 ndarray, info)
        ("shared_focal", points2D_1, points2D_2, pp, opt)   -> (ImagePair, info)
    Returns the list of results in the same order.  Problems of the same kind advance in groups through ONE launch
    sequence (the problem index is a grid dimension of every kernel); `max_in_flight` host threads inside the library
    work on groups concurrently, each with its own HIP stream.  devices: a list of device indices (or "all") spreads the problems
    over several GPUs from this one process (problem i on devices[i mod len]); None: the calling thread's device.
    The point sets may be GPU tensors / __cuda_array_interface__ objects - for all problems of the call or for none (see Batch)."""
    if devices is not None and any(_on_device(pr[1]) or _on_device(pr[2]) for pr in problems):
        raise ValueError("devices= with device points: the memory belongs to one device (set_device selects it)")
    b = Batch(problems)
    b.run(max_in_flight, devices)
    return b.results()


class RansacBatch:
    """pl_ransac_item descriptors for device-resident problems (`Problem`), marshalled once: `run()` is the C-ABI call
    pl_ransac_batch and nothing else (what bench.py times), `results()` returns what `Problem.run` returns per item."""

    def __init__(self, problems, opts):
        assert len(problems) == len(opts)
        self.items = (L.RansacItem * len(problems))()
        self.keep = []
        for it, pr, opt in zip(self.items, problems, opts):
            o = _robust_options(opt, pr.kind, False)
            inl = np.zeros(max(pr.n, 1), dtype=np.uint8)
            st = L.RansacStats()
            if pr.kind in _POSE_KINDS:
                model = _cpose(CameraPose())
                it.model = C.cast(C.pointer(model), C.c_void_p)
            else:
                model = np.ascontiguousarray(np.eye(3).reshape(9))
                it.model = _ptr(model)
            it.problem = pr._h
            it.opt = C.pointer(o)
            it.inliers = _ptr(inl)
            it.stats = C.pointer(st)
            self.keep.append((pr, o, model, inl, st))

    def run(self, max_in_flight=4, group_size=16):
        L.check(L.lib().pl_ransac_batch(self.items, C.c_size_t(len(self.items)), int(max_in_flight), int(group_size)))

    def stats(self):
        return [k[4] for k in self.keep]

    def results(self, first=None):
        """what `Problem.run` returns, per item (`first`: only the first so many items)"""
        out = []
        for pr, o, model, inl, st in (self.keep if first is None else self.keep[:first]):
            if pr.kind in _POSE_KINDS:
                out.append((_pypose(model), _info(st, inl[: pr.n])))
            else:
                out.append((model.reshape(3, 3).T.copy(), _info(st, inl[: pr.n])))
        return out


def device_math(fn: int, x):
    """Diagnostic (pl_debug_device_math): the device kernels' scalar math on an array - 0: cube of the LM's Nielsen update,
    1: sqrt, 2: reciprocal, 3: cbrt, 4: cos, 5: sin, 6: acos, 7: sine of sincos, 8: cosine of sincos, 9: fp16 bits of
    float32(x) rounded to nearest, 10: float32 value of the fp16 bits x, 11: fp16 bits of the smallest fp16 >= float32(x).
    fp16 bit patterns go in and come out as integer-valued doubles.  An unknown code raises PoseLibAmdError."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.zeros_like(x)
    L.check(L.lib().pl_debug_device_math(int(fn), _ptr(x), C.c_size_t(x.size), _ptr(out)))
    return out


def device_math2(fn: int, x, y=None):
    """Diagnostic (pl_debug_device_math2): the device kernels' two-argument scalar math, element-wise - 0: pl_atan2(x, y), x being
    atan2's first argument; 1: pl_tan(x) (y is not read).  An unknown code raises PoseLibAmdError."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    if y is not None:
        y = np.ascontiguousarray(y, dtype=np.float64)
        if y.shape != x.shape:
            raise ValueError("x and y differ in shape")
    out = np.zeros_like(x)
    L.check(L.lib().pl_debug_device_math2(int(fn), _ptr(x), None if y is None else _ptr(y), C.c_size_t(x.size), _ptr(out)))
    return out


def group_slices(kind: int, n_points: int, iterations: int, launch_chunks: int) -> int:
    """Diagnostic (pl_debug_group_slices): hypothesis slices per chunk of correspondences that a group's scorer launch gives one
    member of `n_points` correspondences with a batch of `iterations` iterations, when the chunks of all active members of the
    launch add up to `launch_chunks`.  Host arithmetic only: works without a device."""
    return L.check(L.lib().pl_debug_group_slices(int(kind), int(n_points), int(iterations), int(launch_chunks)))


def score_shape(kind: int, n_points: int, matrix_core: bool, group_form: bool):
    """Diagnostic (pl_debug_score_shape): (chunks, points per lane) of the streaming scorer - fp32-queue or matrix-core form, single
    launch or group member - for n_points correspondences; a chunk holds 64 * points_per_lane of them.  None where no problem of
    this kind and size is scored on the matrix cores.  Host arithmetic only: works without a device."""
    chunks, per_lane = C.c_uint32(0), C.c_uint32(0)
    rc = L.lib().pl_debug_score_shape(int(kind), int(n_points), int(bool(matrix_core)), int(bool(group_form)), C.byref(chunks),
                                      C.byref(per_lane))
    if rc == L.PL_ERR_UNSUPPORTED:
        return None
    L.check(rc)
    return chunks.value, per_lane.value


def score_stream_group(members):
    """Diagnostic (pl_debug_score_stream_ex, route 2): the group form of the streaming scorers.  members: up to four
    (problem, models, max_error, slices) of one kind (0 - 3), slices 0 = the group's own rule; models as Problem.score_stream takes
    them.  One launch scores them all behind an inactive table slot.  Returns ([{"counts", "scores", "path", "slices", "chunks"}
    per member], words the launch changed in the inactive slot's buffers - which must be 0)."""
    arr = (L.DebugScoreMember * max(len(members), 1))()
    keep = []
    for i, (problem, models, max_error, slices) in enumerate(members):
        n, flat = problem._flat_models(models)
        cnt = np.zeros(max(n, 1), dtype=np.uint32)
        sc = np.zeros(max(n, 1), dtype=np.float64)
        keep.append((n, flat, cnt, sc))
        arr[i] = L.DebugScoreMember(problem._h, _ptr(flat), n, float(max_error), _ptr(cnt), _ptr(sc), int(slices), 0, 0, 0)
    idle = C.c_uint32(0)
    L.check(L.lib().pl_debug_score_stream_ex(2, arr, C.c_size_t(len(members)), C.byref(idle)))
    out = [{"counts": cnt[:n], "scores": sc[:n], "path": arr[i].path_used, "slices": arr[i].slices_used, "chunks": arr[i].chunks}
           for i, (n, _, cnt, sc) in enumerate(keep)]
    return out, idle.value


def sampler_shape(K: int, N: int, B: int, window: int = 0):
    """Diagnostic (pl_debug_sampler_shape): the device sampler for B iterations of samples of K out of N - {"window": positions a batch
    step evaluates (the driver's, or `window`), "build": "small" | "large" as the launcher picks it for (window, N, K), "small" /
    "large": {"flags", "doubling", "segments"} capacities of either build of the orbit kernel, "tile": positions per tile of its
    ordered append}.  Host arithmetic only: works without a device."""
    s = L.DebugSamplerShape()
    L.check(L.lib().pl_debug_sampler_shape(int(K), int(N), int(B), int(window), C.byref(s)))
    return {"window": int(s.window), "build": "small" if s.build == 1 else "large", "tile": int(s.tile),
            "small": {"flags": s.small_flags, "doubling": s.small_doubling, "segments": s.small_segments},
            "large": {"flags": s.large_flags, "doubling": s.large_doubling, "segments": s.large_segments}}


_SAMPLER_BUILDS = {None: 0, "small": 1, "large": 2}


def sample_positions(K: int, members, build=None, group: bool = False):
    """Diagnostic (pl_debug_sample_positions): the device sampler's kernels on their own.  members: up to four dicts {"seed",
    "pos_base", "N", "B", "M" (0 / absent: the driver's window), "planted" (absent: the window is drawn; else the delta table itself,
    M bytes, and only the orbit kernel runs)}.  build: None - the launcher's choice -, "small" or "large".  group False: one
    single-problem launch per member; True: all members in one launch of the group form, behind an inactive table slot.  Returns
    ([{"positions", "delta", "flagbits" (the bitmap's ceil(M / 64) words), "guard" (the words behind them), "pos_after",
    "orbit_error", "M", "build", "delta_guard", "ctl_clear"} per member], words the launch changed in the inactive slot's buffers -
    which must be 0)."""
    arr = (L.DebugSamplerMember * max(len(members), 1))()
    keep = []
    for i, m in enumerate(members):
        planted = m.get("planted")
        if planted is not None:
            planted = np.ascontiguousarray(planted, dtype=np.uint8)
            M = int(planted.size)
            if m.get("M", 0) not in (0, M):
                raise ValueError("a planted table has M bytes")
        else:
            M = int(m.get("M", 0)) or sampler_shape(K, m["N"], m["B"])["window"]
        pos = np.zeros(max(int(m["B"]), 1), dtype=np.uint32)
        cap = M if M < (1 << 31) else 0  # (a longer window is refused before anything is written)
        delta = np.zeros(cap + 1, dtype=np.uint8)
        bits = np.zeros(cap // 64 + 2, dtype=np.uint64)
        keep.append((planted, pos, delta, bits))
        arr[i] = L.DebugSamplerMember(int(m.get("seed", 0)), int(m.get("pos_base", 0)), int(m["N"]), int(m["B"]), M,
                                      None if planted is None else _ptr(planted), _ptr(pos), _ptr(delta), _ptr(bits))
    idle = C.c_uint32(0)
    L.check(L.lib().pl_debug_sample_positions(2 if group else 0, int(K), _SAMPLER_BUILDS[build], arr, C.c_size_t(len(members)),
                                              C.byref(idle)))
    out = []
    for i, (_, pos, delta, bits) in enumerate(keep):
        a = arr[i]
        words = (a.M_used + 63) // 64
        out.append({"positions": pos, "delta": delta[:a.M_used], "flagbits": bits[:words], "guard": bits[words:a.M_used // 64 + 2],
                    "pos_after": int(a.pos_after), "orbit_error": int(a.orbit_error), "M": int(a.M_used),
                    "build": "small" if a.build_used == 1 else "large", "delta_guard": bool(a.delta_guard),
                    "ctl_clear": bool(a.ctl_clear)})
    return out, idle.value


def score_prune_gate(kind: int, n_points: int, iterations: int) -> bool:
    """Diagnostic (pl_debug_score_prune_gate): whether a batch step of `iterations` iterations of such a problem scores in the
    pruned form.  Host arithmetic only: works without a device."""
    return bool(L.check(L.lib().pl_debug_score_prune_gate(int(kind), int(n_points), int(iterations))))


def lm_route(kind: int, n_points: int, max_iterations: int = 100):
    """Diagnostic (pl_debug_lm_route): (route, slices) of one camera-less refinement job under the current LM mode and latency
    setting - route 0 k_lm, 1 k_lm_ordered, 2 k_lm2 on `slices` workgroups.  Host arithmetic only: works without a device."""
    slices = C.c_uint32(0)
    return L.check(L.lib().pl_debug_lm_route(int(kind), int(n_points), int(max_iterations), C.byref(slices))), slices.value


def score_pruned(members, route=0):
    """Diagnostic (pl_debug_score_pruned): the pruned form of the matrix-core absolute-pose scorer on caller-given lists.
    members: (problem, models, max_error, init_max, init_min) - one for route 0 (single launches), up to four for route 2 (group
    launches behind an inactive slot).  Returns ([{"counts", "scores", "kept", "cand", "cstar", "chunks", "chunk_points", "lead",
    "lead_max", "lead_min", "num_live", "num_selected", "num_preselected", "slices"} per member], words changed in the inactive slot
    - which must be 0)."""
    arr = (L.DebugPruneMember * max(len(members), 1))()
    keep = []
    cap = 4096
    for i, (problem, models, max_error, init_max, init_min) in enumerate(members):
        n, flat = problem._flat_models(models)
        cnt = np.zeros(max(n, 1), dtype=np.uint32)
        sc = np.zeros(max(n, 1), dtype=np.float64)
        kp = np.zeros(max(n, 1), dtype=np.uint8)
        cand = np.zeros(cap, dtype=np.uint32)
        keep.append((n, flat, cnt, sc, kp, cand))
        arr[i] = L.DebugPruneMember(problem._h, _ptr(flat), n, float(max_error), float(init_min), int(init_max), cap, _ptr(cnt),
                                    _ptr(sc), _ptr(kp), _ptr(cand))
    idle = C.c_uint32(0)
    L.check(L.lib().pl_debug_score_pruned(int(route), arr, C.c_size_t(len(members)), C.byref(idle)))
    out = []
    for i, (n, _, cnt, sc, kp, cand) in enumerate(keep):
        a = arr[i]
        out.append({"counts": cnt[:n], "scores": sc[:n], "kept": kp[:n].astype(bool), "cand": cand[:min(a.num_cand, cap)].copy(),
                    "num_cand": a.num_cand, "cstar": a.cstar, "chunks": a.chunks, "chunk_points": a.chunk_points, "lead": a.lead,
                    "lead_max": a.lead_max, "lead_min": a.lead_min, "num_live": a.num_live, "num_selected": a.num_selected, "num_preselected": a.num_preselected,
                    "slices": a.slices})
    return out, idle.value


def score_survivors(members, route=0):
    """Diagnostic (pl_debug_score_survivors): the count launch of the pruned scorer alone, over the whole list and every chunk.
    members: (problem, models, max_error) - one for route 0, up to four for route 2.  Returns ([{"survivors": (chunks, n) uint32,
    "chunks", "chunk_points", "num_live", "slices"} per member], words changed in the inactive slot, words changed behind the live
    lists' ends - both must be 0)."""
    arr = (L.DebugPruneMember * max(len(members), 1))()
    outs = (C.c_void_p * max(len(members), 1))()
    keep = []
    for i, (problem, models, max_error) in enumerate(members):
        n, flat = problem._flat_models(models)
        chunks = score_shape(problem.kind, problem.n, True, route == 2)[0]
        sv = np.zeros((chunks, max(n, 1)), dtype=np.uint32)
        keep.append((n, flat, sv))
        arr[i] = L.DebugPruneMember(problem._h, _ptr(flat), n, float(max_error))
        outs[i] = sv.ctypes.data
    idle, guard = C.c_uint32(0), C.c_uint32(0)
    L.check(L.lib().pl_debug_score_survivors(int(route), arr, C.c_size_t(len(members)), outs, C.byref(idle), C.byref(guard)))
    out = []
    for i, (n, _, sv) in enumerate(keep):
        a = arr[i]
        assert a.chunks == sv.shape[0], (a.chunks, sv.shape)
        out.append({"survivors": sv[:, :n], "chunks": a.chunks, "chunk_points": a.chunk_points, "num_live": a.num_live, "slices": a.slices})
    return out, idle.value, guard.value


def score_bounded(members, route=0, columns=False):
    """Diagnostic (pl_debug_score_bounded): the pruned scorer as a group's batch step runs it, bound tier included, on caller-given
    lists.  members and routes as score_pruned.  Returns ([score_pruned's fields and "bound_counts", "bound_scores", "tiers" per
    member], words changed in the inactive slot, words changed behind the live lists' ends - both must be 0).  columns
    (pl_debug_score_bounded_columns): also "columns", the (chunks, n) words of the count columns as the launches left them."""
    arr = (L.DebugPruneMember * max(len(members), 1))()
    bcs, bss, trs, cls = ((C.c_void_p * max(len(members), 1))() for _ in range(4))
    keep = []
    cap = 4096
    for i, (problem, models, max_error, init_max, init_min) in enumerate(members):
        n, flat = problem._flat_models(models)
        cnt = np.zeros(max(n, 1), dtype=np.uint32)
        sc = np.zeros(max(n, 1), dtype=np.float64)
        kp = np.zeros(max(n, 1), dtype=np.uint8)
        cand = np.zeros(cap, dtype=np.uint32)
        bc = np.zeros(max(n, 1), dtype=np.uint32)
        bs = np.zeros(max(n, 1), dtype=np.float64)
        tr = np.zeros(max(n, 1), dtype=np.uint8)
        keep.append((n, flat, cnt, sc, kp, cand, bc, bs, tr))
        arr[i] = L.DebugPruneMember(problem._h, _ptr(flat), n, float(max_error), float(init_min), int(init_max), cap, _ptr(cnt),
                                    _ptr(sc), _ptr(kp), _ptr(cand))
        bcs[i], bss[i], trs[i] = bc.ctypes.data, bs.ctypes.data, tr.ctypes.data
        if columns:
            cl = np.zeros((score_shape(problem.kind, problem.n, True, route == 2)[0], max(n, 1)), dtype=np.uint32)
            keep[-1] += (cl,)
            cls[i] = cl.ctypes.data
    idle, guard = C.c_uint32(0), C.c_uint32(0)
    if columns:
        L.check(L.lib().pl_debug_score_bounded_columns(int(route), arr, C.c_size_t(len(members)), bcs, bss, trs, cls, C.byref(idle),
                                                       C.byref(guard)))
    else:
        L.check(L.lib().pl_debug_score_bounded(int(route), arr, C.c_size_t(len(members)), bcs, bss, trs, C.byref(idle), C.byref(guard)))
    out = []
    for i, (n, _, cnt, sc, kp, cand, bc, bs, tr, *cl) in enumerate(keep):
        a = arr[i]
        out.append({"counts": cnt[:n], "scores": sc[:n], "kept": kp[:n].astype(bool), "cand": cand[:min(a.num_cand, cap)].copy(),
                    "num_cand": a.num_cand, "cstar": a.cstar, "chunks": a.chunks, "chunk_points": a.chunk_points, "lead": a.lead,
                    "lead_max": a.lead_max, "lead_min": a.lead_min, "num_live": a.num_live, "num_selected": a.num_selected,
                    "num_preselected": a.num_preselected, "slices": a.slices, "bound_counts": bc[:n], "bound_scores": bs[:n],
                    "tiers": tr[:n]})
        if cl:
            assert a.chunks == cl[0].shape[0], (a.chunks, cl[0].shape)
            out[-1]["columns"] = cl[0][:, :n]
    return out, idle.value, guard.value


def ransac_batch(problems, opts, max_in_flight=4, group_size=16):
    """Many device-resident problems in one call (pl_ransac_batch): results of `problems[i].run(opts[i])`, bit for bit.
    Problems of the same kind advance in lock-step groups of `group_size` through one launch sequence."""
    b = RansacBatch(problems, opts)
    b.run(max_in_flight, group_size)
    return b.results()


def estimate_fundamental(points2D_1, points2D_2, opt=None, initial_F=None, scores=None, min_score=None, inliers_out=None):
    return _estimate_matrix("pl_estimate_fundamental", KIND_FUND, points2D_1, points2D_2, opt, initial_F, scores, min_score, inliers_out)


def estimate_homography(points2D_1, points2D_2, opt=None, initial_H=None, scores=None, min_score=None, inliers_out=None):
    return _estimate_matrix("pl_estimate_homography", KIND_HOM, points2D_1, points2D_2, opt, initial_H, scores, min_score, inliers_out)


# ------------------------------------------------------------------------------------------ ransac_* on normalised points
def _ransac(fn, kind, a, b, dim_b, opt, initial):
    a, b = _pts(a, 2), _pts(b, dim_b)
    o = _robust_options(opt, kind, initial is not None)
    n = a.shape[0]
    inl = np.zeros(max(n, 1), dtype=np.uint8)
    st = L.RansacStats()
    if kind in _POSE_KINDS:
        pose = _cpose(initial if initial is not None else CameraPose())
        L.check(getattr(L.lib(), fn)(_ptr(a), _ptr(b), C.c_size_t(n), C.byref(o), C.byref(pose), _ptr(inl), C.byref(st)))
        return _pypose(pose), _info(st, inl[:n])
    M = np.ascontiguousarray((np.eye(3) if initial is None else np.asarray(initial, dtype=np.float64)).T.reshape(9))
    L.check(getattr(L.lib(), fn)(_ptr(a), _ptr(b), C.c_size_t(n), C.byref(o), _ptr(M), _ptr(inl), C.byref(st)))
    return M.reshape(3, 3).T.copy(), _info(st, inl[:n])


def ransac_pnp(x, X, opt=None, initial_pose=None):
    return _ransac("pl_ransac_pnp", KIND_ABS, x, X, 3, opt, initial_pose)


def ransac_1D_radial_pnp(x, X, opt=None, initial_pose=None):
    """ransac_1D_radial_pnp (ransac.cc:388-401): x = pixels relative to the centre of distortion, taken as they are"""
    return _ransac("pl_ransac_1D_radial_pnp", KIND_RAD1D, x, X, 3, opt, initial_pose)


def _uncalibrated_device_args(pts, scores, min_score, inliers_out):
    """the optional arguments the two _dev entry points of unknown cameras share: (scores, mask, n_used) as ctypes arguments, the
    objects that own their memory"""
    sd, keep = _device_scores(scores, pts.n, min_score) if scores is not None else (None, None)
    md, keep_mask = _device_mask(inliers_out, pts.n) if inliers_out is not None else (None, None)
    used = C.c_size_t(0)
    return (None if sd is None else C.byref(sd), None if md is None else C.byref(md), used), (sd, md, keep, keep_mask)


def estimate_1D_radial_absolute_pose(points2D, points3D, opt=None, initial_pose=None, scores=None, min_score=None, inliers_out=None):
    """poselib.estimate_1D_radial_absolute_pose(points2D, points3D, opt, initial_pose) -> (CameraPose, info): absolute pose of a
    camera with unknown radial distortion from pixels relative to the centre of distortion; the pose has t[2] = 0.
    Points on the GPU (float32 / float64, strided rows) are read where they lie; scores / min_score / inliers_out as
    estimate_absolute_pose."""
    on_device = _on_device(points2D) or _on_device(points3D)
    _check_scores_args(on_device, scores, min_score)
    _check_mask_args(on_device, inliers_out)
    if scores is not None and not _on_device(scores):
        return _scored_host(lambda a, b: estimate_1D_radial_absolute_pose(a, b, opt, initial_pose), points2D, points3D, scores, min_score)
    if not on_device:
        return _ransac("pl_estimate_1D_radial_absolute_pose", KIND_RAD1D, points2D, points3D, 3, opt, initial_pose)
    pts = _Points(points2D, points3D, 2, 3)
    o = _robust_options(opt, KIND_RAD1D, initial_pose is not None)
    n = pts.n
    inl = np.zeros(max(n, 1), dtype=np.uint8)
    st = L.RansacStats()
    pose = _cpose(initial_pose if initial_pose is not None else CameraPose())
    (sd, md, used), keep = _uncalibrated_device_args(pts, scores, min_score, inliers_out)
    L.check(L.lib().pl_estimate_1D_radial_absolute_pose_dev(pts.a, pts.b, sd, C.c_size_t(n), C.byref(o), C.byref(pose), _ptr(inl), md,
                                                            C.byref(st), C.byref(used)))
    del keep
    return _pypose(pose), _info(st, inl[:n] if inliers_out is None else inliers_out, n if scores is None else int(used.value))


def ransac_pnpf(x, X, opt=None):
    """robust/ransac.h ransac_pnpf: pose and focal length of a SIMPLE_PINHOLE camera whose principal point is the origin of `x`.
    Returns (Image(pose, Camera SIMPLE_PINHOLE [f, 0, 0]), info)."""
    x, X = _pts(x, 2), _pts(X, 3)
    o = _robust_options(opt, KIND_ABS, False)
    n = x.shape[0]
    inl = np.zeros(max(n, 1), dtype=np.uint8)
    st = L.RansacStats()
    pose = _cpose(CameraPose())
    focal = C.c_double(1.0)
    L.check(L.lib().pl_ransac_pnpf(_ptr(x), _ptr(X), C.c_size_t(n), C.byref(o), C.byref(pose), C.byref(focal), _ptr(inl), C.byref(st)))
    return Image(_pypose(pose), Camera("SIMPLE_PINHOLE", [focal.value, 0.0, 0.0])), _info(st, inl[:n])


class ImagePair:
    """poselib.ImagePair {pose, camera1, camera2} (types.h / pybind types.cc): here always two copies of one SIMPLE_PINHOLE camera"""

    def __init__(self, pose=None, camera1=None, camera2=None):
        self.pose = pose or CameraPose()
        self.camera1 = camera1 or Camera("SIMPLE_PINHOLE", [1.0, 0.0, 0.0])
        self.camera2 = camera2 or Camera("SIMPLE_PINHOLE", list(self.camera1.params))


def _shared_focal_pair(pose, focal, pp):
    return ImagePair(_pypose(pose), Camera("SIMPLE_PINHOLE", [focal, pp[0], pp[1]]), Camera("SIMPLE_PINHOLE", [focal, pp[0], pp[1]]))


def ransac_shared_focal_relpose(x1, x2, opt=None, initial_pair=None):
    """robust/ransac.h:71-73 ransac_shared_focal_relpose: relative pose and the focal length both views share; x1, x2 relative
    to the principal point.  Returns (ImagePair, info)."""
    x1, x2 = _pts(x1, 2), _pts(x2, 2)
    o = _robust_options(opt, KIND_REL, initial_pair is not None)
    n = x1.shape[0]
    inl = np.zeros(max(n, 1), dtype=np.uint8)
    st = L.RansacStats()
    pose = _cpose(initial_pair.pose if initial_pair is not None else CameraPose())
    focal = C.c_double(initial_pair.camera1.focal() if initial_pair is not None else 1.0)
    L.check(L.lib().pl_ransac_shared_focal_relpose(_ptr(x1), _ptr(x2), C.c_size_t(n), C.byref(o), C.byref(pose), C.byref(focal),
                                                   _ptr(inl), C.byref(st)))
    return _shared_focal_pair(pose, focal.value, (0.0, 0.0)), _info(st, inl[:n])


def estimate_shared_focal_relative_pose(points2D_1, points2D_2, pp, opt=None, initial_pair=None, scores=None, min_score=None,
                                        inliers_out=None):
    """robust.h:84-90 estimate_shared_focal_relative_pose: pixel coordinates, principal point pp.  Returns (ImagePair, info).
    Points on the GPU (float32 / float64, strided rows) are read where they lie; scores / min_score / inliers_out as
    estimate_absolute_pose."""
    on_device = _on_device(points2D_1) or _on_device(points2D_2)
    _check_scores_args(on_device, scores, min_score)
    _check_mask_args(on_device, inliers_out)
    if scores is not None and not _on_device(scores):
        return _scored_host(lambda a, b: estimate_shared_focal_relative_pose(a, b, pp, opt, initial_pair), points2D_1, points2D_2,
                            scores, min_score)
    pts = _Points(points2D_1, points2D_2, 2, 2)
    o = _robust_options(opt, KIND_REL, initial_pair is not None)
    n = pts.n
    inl = np.zeros(max(n, 1), dtype=np.uint8)
    st = L.RansacStats()
    pose = _cpose(initial_pair.pose if initial_pair is not None else CameraPose())
    focal = C.c_double(initial_pair.camera1.focal() if initial_pair is not None else 1.0)
    ppa = np.ascontiguousarray(pp, dtype=np.float64)
    if ppa.shape != (2,):
        raise ValueError("pp: expected two numbers")
    if not pts.on_device:
        L.check(L.lib().pl_estimate_shared_focal_relative_pose(pts.a, pts.b, C.c_size_t(n), _ptr(ppa), C.byref(o), C.byref(pose),
                                                               C.byref(focal), _ptr(inl), C.byref(st)))
        return _shared_focal_pair(pose, focal.value, ppa), _info(st, inl[:n])
    (sd, md, used), keep = _uncalibrated_device_args(pts, scores, min_score, inliers_out)
    L.check(L.lib().pl_estimate_shared_focal_relative_pose_dev(pts.a, pts.b, sd, C.c_size_t(n), _ptr(ppa), C.byref(o), C.byref(pose),
                                                               C.byref(focal), _ptr(inl), md, C.byref(st), C.byref(used)))
    del keep
    return (_shared_focal_pair(pose, focal.value, ppa),
            _info(st, inl[:n] if inliers_out is None else inliers_out, n if scores is None else int(used.value)))


class SharedFocalBatch:
    """An array of pl_shared_focal_item_dev records (include/poselib_amd.h) marshalled once: `run()` is the C-ABI call
    pl_estimate_shared_focal_relative_pose_batch_dev and nothing else, `results()` returns what
    estimate_shared_focal_relative_pose returns per pair: [(ImagePair, info)].

    pairs: (points2D_1, points2D_2, pp, opt) each, the point sets GPU tensors or __cuda_array_interface__ objects - the views of a
    matcher's padded (pairs, N, 5) tensor; nothing is copied to the host.  opt may carry "scores" / "min_score" (one confidence
    per row, on the GPU), "inliers_out" (a GPU array of n one-byte elements that receives the mask) and "initial_pair" (a warm
    start: such a pair runs on its own).  Pairs in host memory: estimate_batch with "shared_focal" problems."""

    def __init__(self, pairs):
        cnt = len(pairs)
        self.items = (L.SharedFocalItemDev * max(cnt, 1))()
        self.scores = (L.DeviceScores * max(cnt, 1))()
        self.masks = (L.DeviceMask * max(cnt, 1))()
        self.n_used = (C.c_size_t * max(cnt, 1))()
        self.scored = self.masked = False
        self.keep = []
        self.mask_out = []  # per pair: the caller's inliers_out= object or None
        streams = {}
        for i, (x1, x2, pp, opt) in enumerate(pairs):
            on = (_on_device(x1), _on_device(x2))
            if on == (False, False):
                raise ValueError("SharedFocalBatch takes points on the GPU: pairs in host memory go through estimate_batch "
                                 "(\"shared_focal\" problems)")
            if on != (True, True):
                raise ValueError("one point set is on the GPU and the other in host memory: pass both the same way")
            opt = dict(opt or {})
            init = opt.pop("initial_pair", None)
            scores, min_score = opt.pop("scores", None), opt.pop("min_score", None)
            inliers_out = opt.pop("inliers_out", None)
            _check_scores_args(True, scores, min_score)
            d1, n, keep1 = _device_points(x1, 2, streams)
            d2, n2, keep2 = _device_points(x2, 2, streams)
            if n2 != n:
                raise ValueError(f"the point sets differ in length ({n} and {n2})")
            ppa = np.ascontiguousarray(pp, dtype=np.float64)
            if ppa.shape != (2,):
                raise ValueError("pp: expected two numbers")
            o = _robust_options(opt, KIND_REL, init is not None)
            pose = _cpose(init.pose if init is not None else CameraPose())
            focal = C.c_double(init.camera1.focal() if init is not None else 1.0)
            inl = np.zeros(max(n, 1), dtype=np.uint8)
            st = L.RansacStats()
            keep_s = None
            if scores is not None:
                self.scores[i], keep_s = _device_scores(scores, n, min_score, streams)
                self.scored = True
            if inliers_out is not None:
                self.masks[i], inliers_out = _device_mask(inliers_out, n, streams)
                self.masked = True
            it = self.items[i]
            it.x1, it.x2, it.n = d1, d2, n
            it.pp[0], it.pp[1] = float(ppa[0]), float(ppa[1])
            it.opt, it.pose, it.focal = C.pointer(o), C.pointer(pose), C.pointer(focal)
            it.inliers = _ptr(inl)
            it.stats = C.pointer(st)
            self.keep.append((o, pose, focal, ppa, inl, st, n, scores is not None, (keep1, keep2, keep_s)))
            self.mask_out.append(inliers_out)
        _sync_streams(streams)  # (once per device, not per tensor: the producers' work is complete before run())

    def run(self, max_in_flight=8):
        L.check(L.lib().pl_estimate_shared_focal_relative_pose_batch_dev(
            self.items, self.scores if self.scored else None, self.masks if self.masked else None, self.n_used,
            C.c_size_t(len(self.keep)), C.c_int(int(max_in_flight))))

    def results(self):
        out = []
        for i, (o, pose, focal, ppa, inl, st, n, scored, _) in enumerate(self.keep):
            info = _info(st, inl[:n] if self.mask_out[i] is None else self.mask_out[i], self.n_used[i] if scored else n)
            out.append((_shared_focal_pair(pose, focal.value, ppa), info))
        return out


def estimate_shared_focal_relative_pose_batch(pairs, max_in_flight=8):
    """estimate_shared_focal_relative_pose for many pairs in GPU memory in one call (SharedFocalBatch; include/poselib_amd.h
    pl_estimate_shared_focal_relative_pose_batch_dev): [(ImagePair, info)] in the order of `pairs`."""
    b = SharedFocalBatch(pairs)
    b.run(max_in_flight)
    return b.results()


def refine_shared_focal_relpose(x1, x2, pair, bundle=None):
    """robust/bundle.h:108-111 refine_shared_focal_relpose on all correspondences (relative to the principal point).
    Returns (ImagePair, LM iterations)."""
    x1, x2 = _pts(x1, 2), _pts(x2, 2)
    o = _robust_options({"bundle": bundle or {}}, KIND_REL, False)
    pose = _cpose(pair.pose)
    focal = C.c_double(pair.camera1.focal())
    its = C.c_uint32(0)
    L.check(L.lib().pl_refine_shared_focal_relpose(_ptr(x1), _ptr(x2), C.c_size_t(x1.shape[0]), C.byref(o.bundle), C.byref(pose),
                                                   C.byref(focal), C.byref(its)))
    return _shared_focal_pair(pose, focal.value, (0.0, 0.0)), its.value


def solve_focal_batch(kind, inputs):
    """pl_solve_focal_batch: kind "p35pf" (inputs count x 20: x 4 x 2 | X 4 x 3) or "relpose_6pt_shared_focal" (count x 36: unit
    bearings x1 6 x 3 | x2 6 x 3).  Returns (models count x slots x 8 [q t focal], counts)."""
    k = {"p35pf": 0, "relpose_6pt_shared_focal": 1}[kind]
    a = np.ascontiguousarray(inputs, dtype=np.float64)
    per, slots = (20, 10) if k == 0 else (36, 60)
    if a.ndim != 2 or a.shape[1] != per:
        raise ValueError(f"expected a (count, {per}) array")
    models = np.zeros((a.shape[0], slots, 8))
    counts = np.zeros(max(a.shape[0], 1), dtype=np.uint32)
    L.check(L.lib().pl_solve_focal_batch(C.c_int(k), _ptr(a), C.c_size_t(a.shape[0]), _ptr(models), _ptr(counts)))
    return models, counts[: a.shape[0]]


def p35pf(x, X):
    """solvers/p35pf.h:39-54: four image points relative to the principal point and their 3-D points -> [(CameraPose, focal)]"""
    models, counts = solve_focal_batch("p35pf", np.r_[_pts(x, 2).reshape(-1), _pts(X, 3).reshape(-1)][None, :])
    return [(CameraPose(m[:4], m[4:7]), float(m[7])) for m in models[0, : counts[0]]]


def relpose_6pt_shared_focal(x1, x2):
    """solvers/relpose_6pt_focal.h:12-13: six pairs of unit bearings -> [(CameraPose, focal)] in the reference's order"""
    models, counts = solve_focal_batch("relpose_6pt_shared_focal", np.r_[_pts(x1, 3).reshape(-1), _pts(x2, 3).reshape(-1)][None, :])
    return [(CameraPose(m[:4], m[4:7]), float(m[7])) for m in models[0, : counts[0]]]


def ransac_relpose(x1, x2, opt=None, initial_pose=None):
    return _ransac("pl_ransac_relpose", KIND_REL, x1, x2, 2, opt, initial_pose)


def ransac_fundamental(x1, x2, opt=None, initial_F=None):
    return _ransac("pl_ransac_fundamental", KIND_FUND, x1, x2, 2, opt, initial_F)


def ransac_homography(x1, x2, opt=None, initial_H=None):
    return _ransac("pl_ransac_homography", KIND_HOM, x1, x2, 2, opt, initial_H)


# ------------------------------------------------------------------------------------------ device-resident problems
class Problem:
    """Correspondences uploaded once (SoA in HBM); `run` executes the LO-RANSAC loop on them.
    This is the entry bench.py times: inputs are resident before the timed region starts.
    a, b: host arrays, or GPU tensors (float32 / float64, any row stride) - those are copied into the problem's block on the device."""

    def __init__(self, kind: int, a, b):
        self.kind = kind
        pts = _Points(a, b, 2, 3 if kind in (KIND_ABS, KIND_RAD1D) else 2)
        self.n = pts.n
        self._h = C.c_void_p()
        L.check(pts.fn("pl_problem_create")(kind, pts.a, pts.b, C.c_size_t(self.n), C.byref(self._h)))

    def run(self, opt=None, initial=None):
        o = _robust_options(opt, self.kind, initial is not None)
        inl = np.zeros(max(self.n, 1), dtype=np.uint8)
        st = L.RansacStats()
        if self.kind in _POSE_KINDS:
            model = _cpose(initial if initial is not None else CameraPose())
            L.check(L.lib().pl_ransac_run(self._h, C.byref(o), C.byref(model), _ptr(inl), C.byref(st)))
            return _pypose(model), _info(st, inl[: self.n])
        M = np.ascontiguousarray((np.eye(3) if initial is None else np.asarray(initial, dtype=np.float64)).T.reshape(9))
        L.check(L.lib().pl_ransac_run(self._h, C.byref(o), _ptr(M), _ptr(inl), C.byref(st)))
        return M.reshape(3, 3).T.copy(), _info(st, inl[: self.n])

    def run_sharded(self, opt, rank: int, world: int, allgather, initial=None):
        """ONE problem across `world` GPUs (pl_ransac_run_sharded): every rank holds the same correspondences in its
        own Problem on its own device and calls this with the same options; each evaluates a contiguous share of every
        batch of iterations, and `allgather(send: bytes-like numpy uint8 array, recv: numpy uint8 array of world *
        len(send))` is the collective of the two exchange steps per batch (see poselib_amd.sharding.dist_allgather for the
        torch.distributed form).  All ranks return the same result - the single-device one."""
        o = _robust_options(opt, self.kind, initial is not None)
        inl = np.zeros(max(self.n, 1), dtype=np.uint8)
        st = L.RansacStats()
        errors = []

        def _cb(_user, send, recv, nbytes):
            try:
                s_arr = np.ctypeslib.as_array(C.cast(send, C.POINTER(C.c_uint8)), shape=(nbytes,))
                r_arr = np.ctypeslib.as_array(C.cast(recv, C.POINTER(C.c_uint8)), shape=(nbytes * world,))
                allgather(s_arr, r_arr)
                return 0
            except Exception as e:  # surfaces as PL_ERR_COMM
                errors.append(e)
                return 1

        cb = L.ALLGATHER_FN(_cb)
        shard = L.Shard(rank, world, cb, None)
        if self.kind in _POSE_KINDS:
            model = _cpose(initial if initial is not None else CameraPose())
            rc = L.lib().pl_ransac_run_sharded(self._h, C.byref(o), C.byref(shard), C.byref(model), _ptr(inl), C.byref(st))
            if rc and errors:
                raise errors[0]
            L.check(rc)
            return _pypose(model), _info(st, inl[: self.n])
        M = np.ascontiguousarray((np.eye(3) if initial is None else np.asarray(initial, dtype=np.float64)).T.reshape(9))
        rc = L.lib().pl_ransac_run_sharded(self._h, C.byref(o), C.byref(shard), _ptr(M), _ptr(inl), C.byref(st))
        if rc and errors:
            raise errors[0]
        L.check(rc)
        return M.reshape(3, 3).T.copy(), _info(st, inl[: self.n])

    def score(self, model, max_error):
        """MSAC score + inlier count of one model (the estimators' score_model())."""
        cnt = C.c_uint64(0)
        sc = C.c_double(0.0)
        if self.kind in _POSE_KINDS:
            m = _cpose(model)
            L.check(L.lib().pl_score_model(self._h, C.byref(m), C.c_double(max_error), C.byref(cnt), C.byref(sc)))
        else:
            M = np.ascontiguousarray(np.asarray(model, dtype=np.float64).T.reshape(9))
            L.check(L.lib().pl_score_model(self._h, _ptr(M), C.c_double(max_error), C.byref(cnt), C.byref(sc)))
        return sc.value, cnt.value

    def _flat_models(self, models):
        m = np.ascontiguousarray(models, dtype=np.float64)
        n = m.shape[0]
        if self.kind in _POSE_KINDS:
            assert m.shape == (n, 7)
            return n, np.ascontiguousarray(m.reshape(-1))  # pl_camera_pose = 7 packed doubles
        assert m.shape == (n, 3, 3)
        return n, np.ascontiguousarray(np.transpose(m, (0, 2, 1)).reshape(-1))  # column-major

    def score_stream(self, models, max_error, slices=0):
        """Diagnostic (pl_debug_score_stream): a list of models through the streaming scorer of the main loop, i.e.
        through the conservative pre-filter in front of the exact evaluation.  models: (n, 7) array of q, t for pose
        problems, (n, 3, 3) matrices otherwise.  Returns (counts, scores, path) with path 2 = matrix-core filter,
        1 = fp32 filter, 0 = no filter.  slices > 0 (pl_debug_score_stream_ex, route 0): a grid of exactly that many
        workgroups per chunk of correspondences instead of the entry's own rule."""
        n, flat = self._flat_models(models)
        cnt = np.zeros(max(n, 1), dtype=np.uint32)
        sc = np.zeros(max(n, 1), dtype=np.float64)
        if slices:
            m = L.DebugScoreMember(self._h, _ptr(flat), n, float(max_error), _ptr(cnt), _ptr(sc), int(slices), 0, 0, 0)
            L.check(L.lib().pl_debug_score_stream_ex(0, C.byref(m), C.c_size_t(1), None))
            assert m.slices_used == int(slices) or n == 0
            return cnt[:n], sc[:n], m.path_used
        path = C.c_int32(0)
        L.check(L.lib().pl_debug_score_stream(self._h, _ptr(flat), C.c_size_t(n), C.c_double(max_error), _ptr(cnt),
                                              _ptr(sc), C.byref(path)))
        return cnt[:n], sc[:n], path.value

    def refine(self, model, bundle_opt=None, camera=None, mask=None):
        """bundle_adjust / refine_relpose / refine_fundamental / refine_homography on the resident points."""
        o = _robust_options({"bundle": bundle_opt or {}}, self.kind, False).bundle
        cam = None if camera is None else _as_camera(camera)._c()
        it = C.c_uint32(0)
        m8 = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        args_tail = (C.byref(cam) if cam is not None else None, None if m8 is None else _ptr(m8))
        if self.kind in _POSE_KINDS:
            m = _cpose(model)
            L.check(L.lib().pl_refine_model(self._h, C.byref(o), *args_tail, C.byref(m), C.byref(it)))
            return _pypose(m), it.value
        M = np.ascontiguousarray(np.asarray(model, dtype=np.float64).T.reshape(9))
        L.check(L.lib().pl_refine_model(self._h, C.byref(o), *args_tail, _ptr(M), C.byref(it)))
        return M.reshape(3, 3).T.copy(), it.value

    def bundle_adjust(self, pose, camera, bundle_opt=None, mask=None):
        """poselib.bundle_adjust(points2D, points3D, camera, pose, opt) on the resident points (2-D points in pixels):
        refines the pose and - with refine_focal_length / refine_principal_point / refine_extra_params - the camera's
        intrinsics (robust/bundle.cc:93-118).  Returns (pose, camera, LM iterations)."""
        assert self.kind == KIND_ABS
        o = _robust_options({"bundle": bundle_opt or {}}, self.kind, False).bundle
        cam = _as_camera(camera)
        c = cam._c()
        it = C.c_uint32(0)
        m8 = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        m = _cpose(pose)
        L.check(L.lib().pl_bundle_adjust_camera(self._h, C.byref(o), C.byref(c), None if m8 is None else _ptr(m8), C.byref(m),
                                                C.byref(it)))
        return _pypose(m), Camera(cam.model_id, list(c.params[: c.num_params]), cam.width, cam.height), it.value

    def close(self):
        if self._h:
            L.lib().pl_problem_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TangentProblem(Problem):
    """Resident tangent-Sampson relative-pose problem (pl_problem_create_tangent): bearings and un-projection Jacobians of the two
    images' pixels, computed on the device.  x1 / x2 in pixels and the cameras as ransac_relpose(x1, x2, camera1, camera2, ...) takes
    them (None: the identity camera).  Models are poses, as for KIND_REL."""

    def __init__(self, x1, x2, camera1=None, camera2=None):
        self.kind = KIND_REL  # (how the models are marshalled)
        pts = _Points(x1, x2, 2, 2)
        self.n = pts.n
        self._h = C.c_void_p()
        c1 = None if camera1 is None else _as_camera(camera1)._c()
        c2 = None if camera2 is None else _as_camera(camera2)._c()
        L.check(pts.fn("pl_problem_create_tangent")(pts.a, pts.b, C.c_size_t(self.n), None if c1 is None else C.byref(c1),
                                                    None if c2 is None else C.byref(c2), C.byref(self._h)))


def radial1d_generate(problem, samples, slots_per_iter=4):
    """Diagnostic (pl_debug_radial1d_generate): the generator kernel of a KIND_RAD1D problem on explicit minimal samples (B, 5).
    Returns (records (B, slots, 16), counts (B,), (models counted, NaN models, overflow flag))."""
    idx = np.ascontiguousarray(samples, dtype=np.uint32).reshape(-1, 5)
    B = idx.shape[0]
    out = np.zeros((B, int(slots_per_iter), 24))
    cnt = np.zeros(B, dtype=np.uint32)
    tot = np.zeros(3, dtype=np.uint32)
    L.check(L.lib().pl_debug_radial1d_generate(problem._h, _ptr(idx), C.c_size_t(B), C.c_uint32(int(slots_per_iter)), _ptr(out), _ptr(cnt),
                                               _ptr(tot)))
    return out[:, :, :16].copy(), cnt, tuple(int(v) for v in tot)


def debug_generate(problem, samples=None, seed=0, pos_base=0, positions=None, slots_per_iter=None, real_focal_check=False, route=0):
    """Diagnostic (pl_debug_generate): the generator of the main loop on a resident problem (Problem of kind 0, 1, 2, 3, 5 or a
    TangentProblem).  Either explicit `samples` (B, K) or `positions` (B,) of the device's own sampler with `seed` / `pos_base`.
    route 0: single-problem launch, 1: single-kernel 5-point generator, 2: group form (two members: all B iterations, and the first
    ceil(B / 3) with buffers of their own).  Returns a list with one dict per member: records (B, slots, 24), num_models (B,),
    nan_bits (B,), blk_tot / blk_nan (ceil(B / 1024),), overflow; the group form's dicts also carry inactive_writes."""
    tangent = isinstance(problem, TangentProblem)
    kind = problem.kind
    K = {KIND_ABS: 3, KIND_REL: 5, KIND_FUND: 7, KIND_HOM: 4, KIND_RAD1D: 5}[kind]
    maxm = {KIND_ABS: 4, KIND_REL: 40, KIND_FUND: 3, KIND_HOM: 1, KIND_RAD1D: 4}[kind]
    slots = maxm if slots_per_iter is None else int(slots_per_iter)
    idx = None if samples is None else np.ascontiguousarray(samples, dtype=np.uint32).reshape(-1, K)
    pos = None if positions is None else np.ascontiguousarray(positions, dtype=np.uint32).reshape(-1)
    B = idx.shape[0] if idx is not None else 0 if pos is None else pos.shape[0]
    members = 2 if route == 2 else 1
    nblk = (B + 1023) // 1024
    rec = np.zeros((members, B, max(slots, 1), 24))
    cnt = np.zeros((members, max(B, 1)), dtype=np.uint32)
    bits = np.zeros((members, max(B, 1)), dtype=np.uint32)
    tot = np.zeros((members, max(nblk, 1)), dtype=np.uint32)
    nan = np.zeros((members, max(nblk, 1)), dtype=np.uint32)
    flags = np.zeros(3, dtype=np.uint32)
    L.check(L.lib().pl_debug_generate(problem._h, None if idx is None else _ptr(idx), C.c_uint64(int(seed)), C.c_uint64(int(pos_base)),
                                      None if pos is None else _ptr(pos), C.c_size_t(B), C.c_uint32(slots), C.c_int(int(bool(real_focal_check))),
                                      C.c_int(int(route)), _ptr(rec), _ptr(cnt), _ptr(bits) if kind == KIND_ABS and not tangent else None,
                                      _ptr(tot), _ptr(nan), _ptr(flags)))
    out = []
    for m in range(members):
        d = {"records": rec[m], "num_models": cnt[m, :B], "nan_bits": bits[m, :B], "blk_tot": tot[m, :nblk], "blk_nan": nan[m, :nblk],
             "overflow": int(flags[m])}
        if route == 2:
            d["inactive_writes"] = int(flags[2])
        out.append(d)
    return out


FOCAL_STAGE_SAMPLE = {KIND_ABS: 4, KIND_FUND: 6}
FOCAL_STAGE_MAX_MODELS = {KIND_ABS: 10, KIND_FUND: 60}


def debug_focal_stage(stage, members, group=False, workgroup_per_model=False):
    """Diagnostic (pl_debug_focal_stage): one stage - "generate", "score" or "mask" - of the focal-length estimators' kernels through
    the production launchers: Problem(KIND_ABS) runs the pnpf kernels, Problem(KIND_FUND) the shared-focal ones.  `members`: a dict
    (or, with group=True, a list of up to 8) with "problem" and, by stage,
      generate  "samples" (B, K) or "positions" (B,) with "seed" / "pos_base"; "max_focal" (default -1: no bound)
      score     "models" (S, 8) [q t f], "thr2"; optional "num_models" (S / max_models,) gate, "as_tasks"
      mask      "model" (8,), "thr2"
    and optionally "idle" (wired with no work over real buffers) and "capacity" (extent of the output buffers, default: the member's
    own).  Returns one dict per member with the whole buffers, prefilled with 0xffffffff (counters) / 0x5a bytes (the rest):
    models, num_models, host_models, host_num_models | counts, sums | mask, host_mask (uint8)."""
    st = {"generate": 0, "score": 1, "mask": 2}[stage]
    single = isinstance(members, dict)
    ms = [members] if single else list(members)
    rec = (L.FocalStageMember * max(len(ms), 1))()
    keep, outs = [], []
    for r, m in zip(rec, ms):
        prob = m["problem"]
        K, maxm = FOCAL_STAGE_SAMPLE.get(prob.kind, 4), FOCAL_STAGE_MAX_MODELS.get(prob.kind, 10)
        r.problem = prob._h
        r.idle = int(bool(m.get("idle", False)))
        r.as_tasks = int(bool(m.get("as_tasks", False)))
        r.seed, r.pos_base = int(m.get("seed", 0)), int(m.get("pos_base", 0))
        r.max_focal, r.thr2 = float(m.get("max_focal", -1.0)), float(m.get("thr2", 0.0))
        out = {}
        if st == 0:
            idx = None if m.get("samples") is None else np.ascontiguousarray(m["samples"], dtype=np.uint32).reshape(-1, K)
            pos = None if m.get("positions") is None else np.ascontiguousarray(m["positions"], dtype=np.uint32).reshape(-1)
            count = int(m["count"]) if "count" in m else idx.shape[0] if idx is not None else 0 if pos is None else pos.shape[0]
            cap = int(m.get("capacity", max(count, 1)))
            out = {"models": np.zeros((cap, maxm, 8)), "num_models": np.zeros(cap, dtype=np.uint32),
                   "host_models": np.zeros((cap, maxm, 8)), "host_num_models": np.zeros(cap, dtype=np.uint32)}
            r.samples = None if idx is None else _ptr(idx)
            r.positions = None if pos is None else _ptr(pos)
            r.out_models, r.out_num_models = _ptr(out["models"]), _ptr(out["num_models"])
            r.out_host_models, r.out_host_num_models = _ptr(out["host_models"]), _ptr(out["host_num_models"])
            keep += [idx, pos]
        elif st == 1:
            mod = None if m.get("models") is None else np.ascontiguousarray(m["models"], dtype=np.float64).reshape(-1, 8)
            gate = None if m.get("num_models") is None else np.ascontiguousarray(m["num_models"], dtype=np.uint32).reshape(-1)
            count = int(m["count"]) if "count" in m else 0 if mod is None else mod.shape[0]
            cap = int(m.get("capacity", max(count, 1)))
            out = {"counts": np.zeros(cap, dtype=np.uint32), "sums": np.zeros(cap)}
            r.models = None if mod is None else _ptr(mod)
            r.num_models = None if gate is None else _ptr(gate)
            r.out_counts, r.out_sums = _ptr(out["counts"]), _ptr(out["sums"])
            keep += [mod, gate]
        else:
            mod = None if m.get("model") is None else np.ascontiguousarray(m["model"], dtype=np.float64).reshape(8)
            count = 0
            cap = int(m.get("capacity", max(prob.n, 1)))
            out = {"mask": np.zeros(cap, dtype=np.uint8), "host_mask": np.zeros(cap, dtype=np.uint8)}
            r.models = None if mod is None else _ptr(mod)
            r.out_mask, r.out_host_mask = _ptr(out["mask"]), _ptr(out["host_mask"])
            keep.append(mod)
        r.count = 0 if r.idle else count
        r.capacity = cap
        outs.append(out)
    L.check(L.lib().pl_debug_focal_stage(C.c_int(st), C.c_int(int(bool(group))), C.c_int(int(bool(workgroup_per_model))), rec,
                                         C.c_size_t(len(ms))))
    del keep
    return outs[0] if single else outs


def inlier_mask(problem, model, max_error):
    """Diagnostic (pl_debug_inlier_mask): the inlier mask of one model on a resident problem."""
    mask = np.zeros(max(problem.n, 1), dtype=np.uint8)
    if problem.kind in _POSE_KINDS:
        m = _cpose(model)
        L.check(L.lib().pl_debug_inlier_mask(problem._h, C.byref(m), C.c_double(max_error), _ptr(mask)))
    else:
        M = np.ascontiguousarray(np.asarray(model, dtype=np.float64).T.reshape(9))
        L.check(L.lib().pl_debug_inlier_mask(problem._h, _ptr(M), C.c_double(max_error), _ptr(mask)))
    return mask[: problem.n].astype(bool)


# ------------------------------------------------------------------------------------------ minimal solvers
def _bearings(x, k):
    x = np.ascontiguousarray(x, dtype=np.float64)
    if x.shape != (k, 3):
        raise ValueError(f"expected {k} bearing vectors of dimension 3")
    return x


def p3p(x, X):
    x, X = _bearings(x, 3), _bearings(X, 3)
    out = (L.CameraPose * 4)()
    n = L.check(L.lib().pl_p3p(_ptr(x), _ptr(X), out))
    return [_pypose(out[i]) for i in range(n)]


def p5lp_radial(x, X):
    """p5lp_radial on five 2-D points (5, 2) and 3-D points (5, 3); the reference's line form is x = (l_y, -l_x)"""
    x, X = np.ascontiguousarray(x, dtype=np.float64), _bearings(X, 5)
    if x.shape != (5, 2):
        raise ValueError("expected 5 points of dimension 2")
    out = (L.CameraPose * 4)()
    n = L.check(L.lib().pl_p5lp_radial(_ptr(x), _ptr(X), out, None))
    return [_pypose(out[i]) for i in range(n)]


def relpose_5pt(x1, x2):
    x1, x2 = _bearings(x1, 5), _bearings(x2, 5)
    out = (L.CameraPose * 40)()
    n = L.check(L.lib().pl_relpose_5pt(_ptr(x1), _ptr(x2), out))
    return [_pypose(out[i]) for i in range(n)]


p5p = relpose_5pt  # alias named by the task statement; the reference exposes relpose_5pt / essential_matrix_5pt


def essential_matrix_5pt(x1, x2):
    x1, x2 = _bearings(x1, 5), _bearings(x2, 5)
    out = np.zeros((10, 9))
    n = L.check(L.lib().pl_essential_matrix_5pt(_ptr(x1), _ptr(x2), _ptr(out)))
    return [out[i].reshape(3, 3).T.copy() for i in range(n)]


def relpose_7pt(x1, x2):
    x1, x2 = _bearings(x1, 7), _bearings(x2, 7)
    out = np.zeros((3, 9))
    n = L.check(L.lib().pl_relpose_7pt(_ptr(x1), _ptr(x2), _ptr(out)))
    return [out[i].reshape(3, 3).T.copy() for i in range(n)]


def homography_4pt(x1, x2):
    x1, x2 = _bearings(x1, 4), _bearings(x2, 4)
    out = np.zeros(9)
    n = L.check(L.lib().pl_homography_4pt(_ptr(x1), _ptr(x2), _ptr(out)))
    return [out.reshape(3, 3).T.copy()] if n else []


def solve_batch(kind: int, first, second, full_records: bool = False):
    """Many minimal problems at once, one GPU lane each.  first/second: (B, K, 3).  Returns
    (records (B, max_models, 16), counts (B,)) — record layout: q[4] t[3] M[9 row-major]; full_records: all 24 doubles of every
    record, the fp32 shadow of the scoring pre-filters included."""
    first = np.ascontiguousarray(first, dtype=np.float64)
    second = np.ascontiguousarray(second, dtype=np.float64)
    B, K = first.shape[0], first.shape[1]
    maxm = {0: 4, 1: 40, 2: 3, 3: 1, 5: 4}[kind]  # (5: p5lp_radial, first = the 2-D points with a third component that is not read)
    inp = np.ascontiguousarray(np.concatenate([first.reshape(B, -1), second.reshape(B, -1)], axis=1))
    out = np.zeros((B, maxm, 24))  # record pitch: 16 fp64 fields + fp32 shadow used by the scoring pre-filter
    cnt = np.zeros(B, dtype=np.uint32)
    L.check(L.lib().pl_solve_batch(kind, _ptr(inp), C.c_size_t(B), _ptr(out), _ptr(cnt)))
    return (out if full_records else out[:, :, :16].copy()), cnt


def _device_points_out(out, n, streams=None):
    """(pl_device_points_out descriptor, the object that owns the memory) of an (n, 2) float64 GPU tensor / __cuda_array_interface__
    object the library writes - a strided view (two columns of a wider block) keeps its strides; nothing is ever copied, so a
    column stride other than 1 is an error.  Synchronisation as _device_points."""
    if _is_torch_tensor(out):
        if not out.is_cuda:
            raise ValueError("out= must be on the GPU when the points are")
        if out.dim() != 2 or out.shape[1] != 2 or int(out.shape[0]) != n:
            raise ValueError(f"out=: expected an ({n}, 2) tensor, got {tuple(out.shape)}")
        if str(out.dtype) != "torch.float64":
            raise ValueError(f"out= must be float64, not {out.dtype}")
        index = out.device.index
        torch = sys.modules.get(type(out).__module__.split(".")[0])
        if index is None and torch is not None:
            index = torch.cuda.current_device()
        if index != _selected_device():
            raise ValueError(f"out= lives on device {index}, this thread selected device {_selected_device()} (set_device)")
        if n > 1 and (out.stride(1) != 1 or out.stride(0) < 2):
            raise ValueError("out= needs a column stride of 1 and a row stride of at least 2 elements")
        if n == 1 and out.stride(1) != 1:
            raise ValueError("out= needs a column stride of 1")
        if torch is not None:
            if streams is None:
                torch.cuda.current_stream(out.device).synchronize()
            else:
                streams.setdefault(index, (torch, out.device))
        row = int(out.stride(0)) if n > 1 else 2
        return L.DevicePointsOut(out.data_ptr() if n else None, row, L.PL_F64, 2), out
    if not _on_device(out):
        raise ValueError("out= must be on the GPU when the points are")
    cai = out.__cuda_array_interface__
    shape = tuple(cai["shape"])
    if len(shape) != 2 or shape[1] != 2 or int(shape[0]) != n:
        raise ValueError(f"out=: expected an ({n}, 2) array, got {shape}")
    if _TYPESTR_DTYPES.get(cai["typestr"], (None, 0))[0] != L.PL_F64:
        raise ValueError(f"out= must be float64, not typestr {cai['typestr']!r}")
    if cai["data"][1]:
        raise ValueError("out= is read-only")
    strides = cai.get("strides")
    row = 2
    if strides is not None:
        if strides[0] % 8 or strides[1] != 8 or (n > 1 and strides[0] < 16):
            raise ValueError("out= needs a column stride of 1 and a row stride of at least 2 elements")
        if n > 1:
            row = strides[0] // 8
    return L.DevicePointsOut(int(cai["data"][0]) if n else None, int(row), L.PL_F64, 2), out


def _new_device_out(points2D, n):
    """a new (n, 2) float64 tensor next to a torch tensor; any other device array cannot be allocated from here"""
    if not _is_torch_tensor(points2D):
        raise ValueError("device points that are no torch tensor need out=: a float64 (N, 2) device array to write")
    torch = sys.modules[type(points2D).__module__.split(".")[0]]
    return torch.empty((n, 2), dtype=torch.float64, device=points2D.device)


def undistort_points(camera, points2D, out=None):
    """Pixels of a distorting camera -> pixels of the distortion-free camera with the same focal lengths and principal
    point (pl_undistort_points: Camera::unproject per point on the device, then fx u + cx, fy v + cy).  The stage in
    front of estimate_homography / estimate_fundamental, which take no camera.

    points2D on the GPU (a torch tensor or a __cuda_array_interface__ object, float32 or float64, strided rows): the result stays
    there (pl_undistort_points_dev) - out= (float64, (N, 2), may be a strided view such as columns 0:2 of an (N, 4) tensor, or
    points2D itself when that is float64) is written and returned; without it a torch tensor gives a new float64 tensor on its
    device, any other device array needs out=.  The values are those of the host call on the same numbers as doubles, bit for bit."""
    if not _on_device(points2D):
        if out is not None:
            raise ValueError("out= goes with points on the GPU; host points return a new array")
        a = _pts(points2D, 2)
        res = np.zeros_like(a)
        c = _as_camera(camera)._c()
        L.check(L.lib().pl_undistort_points(C.byref(c), _ptr(a), C.c_size_t(a.shape[0]), _ptr(res)))
        return res
    streams = {}
    src, n, keep = _device_points(points2D, 2, streams)
    if out is None:
        out = _new_device_out(points2D, n)
    dst, out = _device_points_out(out, n, streams)
    _sync_streams(streams)
    c = _as_camera(camera)._c()
    L.check(L.lib().pl_undistort_points_dev(C.byref(c), C.byref(src), C.c_size_t(n), C.byref(dst)))
    del keep
    return out


def undistort_points_batch(items):
    """undistort_points for many views in one call: items = [(camera, points2D, out_or_None), ...], all on the GPU
    (pl_undistort_points_batch_dev: one launch and one synchronisation for the whole list) or all in host memory (a loop over
    undistort_points).  Returns the list of outputs.  A matcher batch is 2 x pairs views over a handful of cameras."""
    items = [tuple(it) + (None,) * (3 - len(it)) for it in items]
    on = [_on_device(p) for _, p, _ in items]
    if len(set(on)) > 1:
        raise ValueError("host and device items mixed in one call: pass all point sets the same way")
    if not items or not on[0]:
        return [undistort_points(cam, p, o) for cam, p, o in items]
    streams, keep, outs = {}, [], []
    rec = (L.UndistortItemDev * len(items))()
    for k, (cam, p, o) in enumerate(items):
        src, n, owner = _device_points(p, 2, streams)
        if o is None:
            o = _new_device_out(p, n)
        dst, o = _device_points_out(o, n, streams)
        c = _as_camera(cam)._c()
        keep.append((owner, c))
        outs.append(o)
        rec[k].camera = C.pointer(c)
        rec[k].points2D, rec[k].n, rec[k].out = src, n, dst
    _sync_streams(streams)
    L.check(L.lib().pl_undistort_points_batch_dev(rec, C.c_size_t(len(items))))
    del keep
    return outs


def device_count() -> int:
    return L.lib().pl_device_count()


def set_device(i: int):
    L.check(L.lib().pl_set_device(int(i)))
    _tls.device = int(i)


def check_device_points(desc, n: int, cols: int) -> int:
    """Diagnostic (pl_debug_check_device_points): the return code of every check the _dev entry points make on one argument -
    desc: a _lib.DevicePoints, or None for a null descriptor.  No kernel is launched."""
    return L.lib().pl_debug_check_device_points(None if desc is None else C.byref(desc), C.c_size_t(int(n)), int(cols))


def rank_tile(max_n: int) -> int:
    """Diagnostic (pl_debug_rank_tile): the rows one workgroup of the ranking kernel sorts out of LDS in a launch whose largest
    member has max_n rows; larger members take merge passes through global memory."""
    return int(L.lib().pl_debug_rank_tile(C.c_size_t(int(max_n))))


def rank_scores(scores, min_score=None):
    """Diagnostic (pl_debug_rank_scores): the permutation the scored entry points use - the rows of a one-dimensional device
    array with score >= min_score, in descending score, ties in ascending row (score_order is the same rule in numpy).  A list of
    arrays (min_score: one value, or one per array) is ranked by ONE launch sequence of the grouped kernels and returns a list."""
    single = not isinstance(scores, (list, tuple))
    members = [scores] if single else list(scores)
    mins = list(min_score) if isinstance(min_score, (list, tuple)) else [min_score] * len(members)
    if len(mins) != len(members):
        raise ValueError("min_score: one value, or one per member")
    if not all(_on_device(m) for m in members):
        raise ValueError("rank_scores takes device arrays (score_order ranks host arrays)")
    cnt = len(members)
    if cnt == 0:
        return []
    ns = (C.c_size_t * cnt)(*[int(m.shape[0]) for m in members])
    desc = (L.DeviceScores * cnt)()
    keep = []
    for k, (m, lo) in enumerate(zip(members, mins)):
        desc[k], owner = _device_scores(m, ns[k], lo)
        keep.append(owner)
    order = np.zeros(max(sum(ns), 1), dtype=np.uint32)
    kept = (C.c_size_t * cnt)()
    L.check(L.lib().pl_debug_rank_scores(desc, ns, C.c_size_t(cnt), _ptr(order), kept))
    out, at = [], 0
    for k in range(cnt):
        out.append(order[at:at + kept[k]].copy())
        at += ns[k]
    return out[0] if single else out


def point_stats_dev(x1, x2, centroid=True):
    """Diagnostic (pl_debug_point_stats_dev): what the GPU-input front-ends read back in place of the host's passes over the points,
    for two (N, 2) GPU tensors: {"c1", "c2", "scale", "absmax_normalised", "absmax_first"}."""
    pts = _Points(x1, x2, 2, 2)
    if not pts.on_device:
        raise ValueError("point_stats_dev takes GPU tensors")
    out = np.zeros(8)
    L.check(L.lib().pl_debug_point_stats_dev(pts.a, pts.b, C.c_size_t(pts.n), int(bool(centroid)), _ptr(out)))
    return {"c1": out[0:2].copy(), "c2": out[2:4].copy(), "scale": float(out[4]), "absmax_normalised": float(out[5]),
            "absmax_first": float(out[6])}


def point_stats_about_dev(x1, x2=None, centre=(0.0, 0.0)):
    """Diagnostic (pl_debug_point_stats_about_dev): the reduction the device forms of the two estimators of unknown cameras read
    back, for (N, 2) GPU tensors.  x2 given: the mean distance of both sets from `centre` over sqrt(2) (shared focal); x2 None:
    n / sum |x_k| of x1 (1D radial).  Returns {"scale", "absmax"} (absmax: max |coordinate * scale|, radial only)."""
    if not _on_device(x1) or (x2 is not None and not _on_device(x2)):
        raise ValueError("point_stats_about_dev takes GPU tensors")
    d1, n, keep1 = _device_points(x1, 2)
    d2, n2, keep2 = _device_points(x2, 2) if x2 is not None else (None, n, None)
    if n2 != n:
        raise ValueError(f"the point sets differ in length ({n} and {n2})")
    out = np.zeros(2)
    L.check(L.lib().pl_debug_point_stats_about_dev(C.byref(d1), None if d2 is None else C.byref(d2), C.c_size_t(n), float(centre[0]),
                                                   float(centre[1]), _ptr(out)))
    del keep1, keep2
    return {"scale": float(out[0]), "absmax": float(out[1])}


def point_stats_group_dev(pairs, centroid=True):
    """Diagnostic (pl_debug_point_stats_group_dev): point_stats_dev for a list of (x1, x2) pairs of device point sets at once,
    through the grouped kernels of pl_estimate_batch_dev - one list entry per pair."""
    keep = [_Points(x1, x2, 2, 2) for x1, x2 in pairs]
    if not all(p.on_device for p in keep):
        raise ValueError("point_stats_group_dev takes device points")
    cnt = len(keep)
    d1 = (L.DevicePoints * max(cnt, 1))(*[p.keep[0] for p in keep])
    d2 = (L.DevicePoints * max(cnt, 1))(*[p.keep[1] for p in keep])
    ns = (C.c_size_t * max(cnt, 1))(*[p.n for p in keep])
    out = np.zeros((max(cnt, 1), 8))
    L.check(L.lib().pl_debug_point_stats_group_dev(d1, d2, ns, C.c_size_t(cnt), int(bool(centroid)), _ptr(out)))
    return [{"c1": o[0:2].copy(), "c2": o[2:4].copy(), "scale": float(o[4]), "absmax_normalised": float(o[5]),
             "absmax_first": float(o[6])} for o in out[:cnt]]


def point_stats_about_group_dev(pairs, centres):
    """Diagnostic (pl_debug_point_stats_about_group_dev): point_stats_about_dev's shared-focal reduction for a list of (x1, x2)
    pairs of device point sets at once, every pair about its own centre, through the grouped kernels of
    pl_estimate_shared_focal_relative_pose_batch_dev - the list of scales."""
    keep = [_Points(x1, x2, 2, 2) for x1, x2 in pairs]
    if not all(p.on_device for p in keep):
        raise ValueError("point_stats_about_group_dev takes device points")
    cnt = len(keep)
    cen = np.ascontiguousarray(centres, dtype=np.float64).reshape(-1, 2)
    if cen.shape[0] != cnt:
        raise ValueError(f"{cen.shape[0]} centres for {cnt} pairs")
    d1 = (L.DevicePoints * max(cnt, 1))(*[p.keep[0] for p in keep])
    d2 = (L.DevicePoints * max(cnt, 1))(*[p.keep[1] for p in keep])
    ns = (C.c_size_t * max(cnt, 1))(*[p.n for p in keep])
    out = np.zeros((max(cnt, 1), 2))
    L.check(L.lib().pl_debug_point_stats_about_group_dev(d1, d2, ns, _ptr(cen), C.c_size_t(cnt), _ptr(out)))
    return [float(o[0]) for o in out[:cnt]]


def set_lm_mode(mode) -> int:
    """Summation order of the non-linear refinements.  0 / False (default): the reference's order up to 256 correspondences and
    tree order beyond for poses and homographies, the reference's order at every size for fundamental matrices (the sign of a
    refined F hangs on the bits of the refinement's input); 1 / True: the reference's order at every size for every estimator
    (bit-identical refined models, slower); 2: tree order beyond 256 correspondences for every estimator.  Returns the previous mode."""
    return int(L.lib().pl_set_lm_mode(int(mode)))
