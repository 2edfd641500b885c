"""ctypes binding of poselib_amd/lib/libposelib_amd.so (the C-ABI in include/poselib_amd.h).

The shared library is the product: hand-written HIP kernels for gfx950 plus the host driver.
There is no Python/CPU implementation behind this module — if the library is missing or no HIP
device is usable, calls raise.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

_PKG = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_PKG, "csrc")
LIB_PATH = os.path.join(_PKG, "lib", "libposelib_amd.so")
if os.environ.get("POSELIB_AMD_LIB"):  # development: another build of the same C-ABI (A/B timing of kernel variants)
    LIB_PATH = os.environ["POSELIB_AMD_LIB"]

u64, i32, u32, f64 = C.c_uint64, C.c_int32, C.c_uint32, C.c_double

PL_OK, PL_ERR_NO_DEVICE, PL_ERR_HIP, PL_ERR_INVALID, PL_ERR_UNSUPPORTED, PL_ERR_COMM = 0, -1, -2, -3, -4, -5


class RansacOptions(C.Structure):
    _fields_ = [("max_iterations", u64), ("min_iterations", u64), ("dyn_num_trials_mult", f64), ("success_prob", f64),
                ("seed", u64), ("progressive_sampling", i32), ("score_initial_model", i32),
                ("max_prosac_iterations", u64)]


class BundleOptions(C.Structure):
    _fields_ = [("max_iterations", u64), ("loss_type", i32), ("lambda_update", i32), ("damping", i32), ("verbose", i32),
                ("loss_scale", f64), ("gradient_tol", f64), ("step_tol", f64), ("relative_cost_tol", f64),
                ("initial_lambda", f64), ("min_lambda", f64), ("max_lambda", f64), ("lambda_factor", f64),
                ("refine_focal_length", i32), ("refine_extra_params", i32), ("refine_principal_point", i32),
                ("reserved", i32)]


class RobustOptions(C.Structure):
    _fields_ = [("ransac", RansacOptions), ("bundle", BundleOptions), ("max_error", f64), ("real_focal_check", i32),
                ("tangent_sampson", i32), ("estimate_focal_length", i32), ("estimate_extra_params", i32), ("min_fov", f64)]


class RansacStats(C.Structure):
    _fields_ = [("refinements", u64), ("iterations", u64), ("num_inliers", u64), ("inlier_ratio", f64),
                ("model_score", f64), ("hypotheses", u64), ("iterations_evaluated", u64), ("seconds", f64),
                ("score_kernel_ms", f64), ("score_kernel_launches", u32), ("nan_hypotheses", u32)]


class BatchItem(C.Structure):
    pass  # fields set below (needs Camera / RobustOptions)


class Camera(C.Structure):
    _fields_ = [("model_id", i32), ("width", i32), ("height", i32), ("num_params", i32), ("params", f64 * 12)]


class CameraPose(C.Structure):
    _fields_ = [("q", f64 * 4), ("t", f64 * 3)]


BatchItem._fields_ = [("kind", i32), ("status", i32), ("a", C.c_void_p), ("b", C.c_void_p), ("n", C.c_size_t),
                      ("opt", C.POINTER(RobustOptions)), ("camera1", C.POINTER(Camera)), ("camera2", C.POINTER(Camera)),
                      ("model", C.c_void_p), ("inliers", C.c_void_p), ("stats", C.POINTER(RansacStats))]


class BatchReport(C.Structure):  # pl_batch_report
    _fields_ = [("items", C.c_uint64), ("grouped", C.c_uint64), ("focal_grouped", C.c_uint64), ("solo", C.c_uint64),
                ("fallback", C.c_uint64)]


class RansacItem(C.Structure):  # pl_ransac_item
    _fields_ = [("problem", C.c_void_p), ("opt", C.POINTER(RobustOptions)), ("model", C.c_void_p), ("inliers", C.c_void_p),
                ("stats", C.POINTER(RansacStats)), ("status", i32), ("reserved", i32)]


ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t)


class Shard(C.Structure):  # pl_shard
    _fields_ = [("rank", i32), ("world", i32), ("allgather", ALLGATHER_FN), ("user", C.c_void_p)]


class DebugScoreMember(C.Structure):  # pl_debug_score_member
    _fields_ = [("problem", C.c_void_p), ("models", C.c_void_p), ("n", C.c_size_t), ("max_error", f64), ("counts", C.c_void_p),
                ("scores", C.c_void_p), ("slices", u32), ("slices_used", u32), ("chunks", u32), ("path_used", i32)]


class DebugPruneMember(C.Structure):  # pl_debug_prune_member
    _fields_ = [("problem", C.c_void_p), ("models", C.c_void_p), ("n", C.c_size_t), ("max_error", f64), ("init_min", f64),
                ("init_max", u32), ("cand_cap", u32), ("counts", C.c_void_p), ("scores", C.c_void_p), ("kept", C.c_void_p),
                ("cand", C.c_void_p), ("num_cand", u32), ("cstar", u32), ("chunks", u32), ("chunk_points", u32), ("lead", u32),
                ("lead_max", u32), ("num_live", u32), ("num_selected", u32), ("slices", u32), ("num_preselected", u32), ("lead_min", f64)]


class DebugSamplerShape(C.Structure):  # pl_debug_sampler_shape_info
    _fields_ = [("window", u64), ("build", u32), ("tile", u32), ("small_flags", u32), ("small_doubling", u32), ("small_segments", u32),
                ("large_flags", u32), ("large_doubling", u32), ("large_segments", u32)]


class DebugSamplerMember(C.Structure):  # pl_debug_sampler_member
    _fields_ = [("seed", u64), ("pos_base", u64), ("N", u64), ("B", u32), ("M", u32), ("planted", C.c_void_p), ("positions", C.c_void_p),
                ("delta", C.c_void_p), ("flagbits", C.c_void_p), ("pos_after", u64), ("orbit_error", u32), ("M_used", u32),
                ("build_used", u32), ("delta_guard", i32), ("ctl_clear", i32), ("pad", i32)]


class FocalStageMember(C.Structure):  # pl_focal_stage_member
    _fields_ = [("problem", C.c_void_p), ("idle", i32), ("as_tasks", i32), ("count", u32), ("capacity", u32), ("samples", C.c_void_p),
                ("positions", C.c_void_p), ("seed", u64), ("pos_base", u64), ("max_focal", C.c_double), ("thr2", C.c_double),
                ("models", C.c_void_p), ("num_models", C.c_void_p), ("out_models", C.c_void_p), ("out_host_models", C.c_void_p),
                ("out_num_models", C.c_void_p), ("out_host_num_models", C.c_void_p), ("out_counts", C.c_void_p), ("out_sums", C.c_void_p),
                ("out_mask", C.c_void_p), ("out_host_mask", C.c_void_p)]


PL_F64, PL_F32 = 0, 1


class DevicePoints(C.Structure):  # pl_device_points: rows of `cols` contiguous fp32 / fp64 elements in DEVICE memory
    _fields_ = [("data", C.c_void_p), ("row_stride", C.c_int64), ("dtype", i32), ("cols", i32)]


class BatchItemDev(C.Structure):  # pl_batch_item_dev: pl_batch_item with the two host pointers replaced by descriptors (by value)
    _fields_ = [("kind", i32), ("status", i32), ("a", DevicePoints), ("b", DevicePoints), ("n", C.c_size_t),
                ("opt", C.POINTER(RobustOptions)), ("camera1", C.POINTER(Camera)), ("camera2", C.POINTER(Camera)),
                ("model", C.c_void_p), ("inliers", C.c_void_p), ("stats", C.POINTER(RansacStats))]


class DeviceScores(C.Structure):  # pl_device_scores: one confidence per row in DEVICE memory, `stride` elements apart
    _fields_ = [("data", C.c_void_p), ("stride", C.c_int64), ("dtype", i32), ("reserved", i32), ("min_score", f64)]


class DevicePointsOut(C.Structure):  # pl_device_points_out: fp64 rows in DEVICE memory that a call writes (columns 0 and 1)
    _fields_ = [("data", C.c_void_p), ("row_stride", C.c_int64), ("dtype", i32), ("cols", i32)]


class UndistortItemDev(C.Structure):  # pl_undistort_item_dev
    _fields_ = [("status", i32), ("reserved", i32), ("camera", C.POINTER(Camera)), ("points2D", DevicePoints), ("n", C.c_size_t),
                ("out", DevicePointsOut)]


class DeviceMask(C.Structure):  # pl_device_mask: one flag byte per row in DEVICE memory, `stride` BYTES apart
    _fields_ = [("data", C.c_void_p), ("stride", C.c_int64)]


class SharedFocalItemDev(C.Structure):  # pl_shared_focal_item_dev
    _fields_ = [("status", i32), ("reserved", i32), ("x1", DevicePoints), ("x2", DevicePoints), ("n", C.c_size_t), ("pp", f64 * 2),
                ("opt", C.POINTER(RobustOptions)), ("pose", C.POINTER(CameraPose)), ("focal", C.POINTER(f64)), ("inliers", C.c_void_p),
                ("stats", C.POINTER(RansacStats))]


class PoseLibAmdError(RuntimeError):
    pass


def build(force: bool = False, verbose: bool = False) -> str:
    """Compile the HIP library in-tree (hipcc cross-compiles gfx950 without a GPU)."""
    srcs = [os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith((".h", ".hip", ".cc", ".inc", "Makefile"))]
    srcs.append(os.path.join(os.path.dirname(_PKG), "include", "poselib_amd.h"))
    stale = (not os.path.exists(LIB_PATH)) or any(os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs)
    if force or stale:
        cmd = ["make", "-C", _CSRC]
        if not verbose:
            cmd.append("-s")
        subprocess.check_call(cmd)
    return LIB_PATH


_lib = None


def lib():
    """Load the C-ABI library.  Raises if it has not been built (use poselib_amd.build())."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise PoseLibAmdError(
                f"{LIB_PATH} is missing: build it with `python -c 'import poselib_amd; poselib_amd.build()'` "
                "(there is no CPU fallback)")
        # The HIP runtime maps a process's streams onto GPU_MAX_HW_QUEUES hardware queues (4 by default; streams that share
        # a queue run one after the other) and reads the variable at its first call.  The batch entry points keep 8 - 16
        # streams in flight, so this binding - the application layer of a Python process - asks for 16 unless the user
        # chose a value or opted out (POSELIB_AMD_KEEP_ENV=1).  The C library itself never touches the environment.
        if not os.environ.get("POSELIB_AMD_KEEP_ENV"):
            os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
        L = C.CDLL(LIB_PATH)
        _declare(L)
        _lib = L
    return _lib


def _declare(L):
    """argtypes / restype of every C-ABI function (include/poselib_amd.h), so that a bare Python int or None is
    converted to the declared width instead of ctypes' default c_int."""
    vp, sz, dbl, cint = C.c_void_p, C.c_size_t, C.c_double, C.c_int
    P = C.POINTER
    opt, stats, cam, pose = P(RobustOptions), P(RansacStats), P(Camera), P(CameraPose)
    dpts = P(DevicePoints)
    sig = {
        "pl_default_ransac_options": (None, [P(RansacOptions)]),
        "pl_default_bundle_options": (None, [P(BundleOptions)]),
        "pl_default_robust_options": (None, [opt, cint]),
        "pl_device_count": (cint, []),
        "pl_set_lm_mode": (cint, [cint]),
        "pl_set_device": (cint, [cint]),
        "pl_last_error": (C.c_char_p, []),
        "pl_version": (C.c_char_p, []),
        "pl_abi_version": (cint, []),
        "pl_estimate_absolute_pose": (cint, [vp, vp, sz, opt, cam, pose, vp, stats]),
        "pl_estimate_relative_pose": (cint, [vp, vp, sz, cam, cam, opt, pose, vp, stats]),
        "pl_estimate_fundamental": (cint, [vp, vp, sz, opt, vp, vp, stats]),
        "pl_estimate_homography": (cint, [vp, vp, sz, opt, vp, vp, stats]),
        "pl_estimate_absolute_pose_dev": (cint, [dpts, dpts, sz, opt, cam, pose, vp, stats]),
        "pl_estimate_relative_pose_dev": (cint, [dpts, dpts, sz, cam, cam, opt, pose, vp, stats]),
        "pl_estimate_fundamental_dev": (cint, [dpts, dpts, sz, opt, vp, vp, stats]),
        "pl_estimate_homography_dev": (cint, [dpts, dpts, sz, opt, vp, vp, stats]),
        "pl_problem_create_dev": (cint, [cint, dpts, dpts, sz, P(vp)]),
        "pl_problem_create_tangent_dev": (cint, [dpts, dpts, sz, cam, cam, P(vp)]),
        "pl_debug_check_device_points": (cint, [dpts, sz, cint]),
        "pl_debug_point_stats_dev": (cint, [dpts, dpts, sz, cint, vp]),
        "pl_estimate_batch": (cint, [P(BatchItem), sz, cint]),
        "pl_estimate_batch_devices": (cint, [P(BatchItem), sz, P(C.c_int), cint, cint]),
        "pl_estimate_batch_dev": (cint, [P(BatchItemDev), sz, cint]),
        "pl_debug_point_stats_group_dev": (cint, [dpts, dpts, P(sz), sz, cint, vp]),
        "pl_estimate_dev_scored": (cint, [cint, dpts, dpts, P(DeviceScores), sz, opt, cam, cam, vp, vp, stats, P(sz)]),
        "pl_estimate_batch_dev_scored": (cint, [P(BatchItemDev), P(DeviceScores), P(sz), sz, cint]),
        "pl_estimate_dev_masked": (cint, [cint, dpts, dpts, P(DeviceScores), sz, opt, cam, cam, vp, P(DeviceMask), stats, P(sz)]),
        "pl_estimate_batch_dev_masked": (cint, [P(BatchItemDev), P(DeviceScores), P(DeviceMask), P(sz), sz, cint]),
        "pl_debug_rank_scores": (cint, [P(DeviceScores), P(sz), sz, vp, P(sz)]),
        "pl_debug_rank_tile": (cint, [sz]),
        "pl_estimate_shared_focal_relative_pose_dev": (cint, [dpts, dpts, P(DeviceScores), sz, vp, opt, pose, P(dbl), vp, P(DeviceMask), stats,
                                                               P(sz)]),
        "pl_estimate_1D_radial_absolute_pose_dev": (cint, [dpts, dpts, P(DeviceScores), sz, opt, pose, vp, P(DeviceMask), stats, P(sz)]),
        "pl_debug_point_stats_about_dev": (cint, [dpts, dpts, sz, dbl, dbl, vp]),
        "pl_estimate_shared_focal_relative_pose_batch_dev": (cint, [P(SharedFocalItemDev), P(DeviceScores), P(DeviceMask), P(sz), sz, cint]),
        "pl_debug_point_stats_about_group_dev": (cint, [dpts, dpts, P(sz), vp, sz, vp]),
        "pl_last_batch_report": (None, [P(BatchReport)]),
        "pl_ransac_batch": (cint, [P(RansacItem), sz, cint, cint]),
        "pl_undistort_points": (cint, [cam, vp, sz, vp]),
        "pl_undistort_points_dev": (cint, [cam, dpts, sz, P(DevicePointsOut)]),
        "pl_undistort_points_batch_dev": (cint, [P(UndistortItemDev), sz]),
        "pl_ransac_pnp": (cint, [vp, vp, sz, opt, pose, vp, stats]),
        "pl_ransac_pnpf": (cint, [vp, vp, sz, opt, pose, P(dbl), vp, stats]),
        "pl_ransac_relpose": (cint, [vp, vp, sz, opt, pose, vp, stats]),
        "pl_ransac_shared_focal_relpose": (cint, [vp, vp, sz, opt, pose, P(dbl), vp, stats]),
        "pl_solve_focal_batch": (cint, [cint, vp, sz, vp, vp]),
        "pl_p35pf": (cint, [vp, vp, vp, vp]),
        "pl_relpose_6pt_shared_focal": (cint, [vp, vp, vp, vp]),
        "pl_refine_shared_focal_relpose": (cint, [vp, vp, sz, P(BundleOptions), pose, P(dbl), P(C.c_uint32)]),
        "pl_estimate_shared_focal_relative_pose": (cint, [vp, vp, sz, vp, opt, pose, P(dbl), vp, stats]),
        "pl_ransac_fundamental": (cint, [vp, vp, sz, opt, vp, vp, stats]),
        "pl_ransac_homography": (cint, [vp, vp, sz, opt, vp, vp, stats]),
        "pl_problem_create": (cint, [cint, vp, vp, sz, P(vp)]),
        "pl_problem_create_tangent": (cint, [vp, vp, sz, cam, cam, P(vp)]),
        "pl_debug_inlier_mask": (cint, [vp, vp, dbl, vp]),
        "pl_debug_tangent_chunk": (cint, []),
        "pl_debug_radial1d_chunk": (cint, []),
        "pl_debug_group_slices": (cint, [cint, C.c_uint32, C.c_uint32, C.c_uint32]),
        "pl_debug_radial1d_generate": (cint, [vp, vp, sz, C.c_uint32, vp, vp, vp]),
        "pl_debug_generate": (cint, [vp, vp, u64, u64, vp, sz, C.c_uint32, cint, cint, vp, vp, vp, vp, vp, vp]),
        "pl_debug_focal_stage": (cint, [cint, cint, cint, P(FocalStageMember), sz]),
        "pl_estimate_1D_radial_absolute_pose": (cint, [vp, vp, sz, opt, pose, vp, stats]),
        "pl_ransac_1D_radial_pnp": (cint, [vp, vp, sz, opt, pose, vp, stats]),
        "pl_p5lp_radial": (cint, [vp, vp, P(CameraPose), P(cint)]),
        "pl_problem_destroy": (None, [vp]),
        "pl_ransac_run": (cint, [vp, opt, vp, vp, stats]),
        "pl_ransac_run_sharded": (cint, [vp, opt, P(Shard), vp, vp, stats]),
        "pl_score_model": (cint, [vp, vp, dbl, P(C.c_uint64), P(dbl)]),
        "pl_debug_score_stream": (cint, [vp, vp, sz, dbl, vp, vp, P(C.c_int32)]),
        "pl_debug_score_shape": (cint, [cint, C.c_uint32, cint, cint, P(C.c_uint32), P(C.c_uint32)]),
        "pl_debug_score_stream_ex": (cint, [cint, P(DebugScoreMember), sz, P(C.c_uint32)]),
        "pl_debug_score_pruned": (cint, [cint, P(DebugPruneMember), sz, P(C.c_uint32)]),
        "pl_debug_score_survivors": (cint, [cint, P(DebugPruneMember), sz, P(C.c_void_p), P(C.c_uint32), P(C.c_uint32)]),
        "pl_debug_score_bounded": (cint, [cint, P(DebugPruneMember), sz, P(C.c_void_p), P(C.c_void_p), P(C.c_void_p), P(C.c_uint32),
                                           P(C.c_uint32)]),
        "pl_debug_score_bounded_columns": (cint, [cint, P(DebugPruneMember), sz, P(C.c_void_p), P(C.c_void_p), P(C.c_void_p), P(C.c_void_p),
                                                   P(C.c_uint32), P(C.c_uint32)]),
        "pl_debug_score_prune_gate": (cint, [cint, C.c_uint32, C.c_uint32]),
        "pl_debug_lm_route": (cint, [cint, C.c_uint32, u64, P(C.c_uint32)]),
        "pl_debug_sampler_shape": (cint, [cint, u64, C.c_uint32, u64, P(DebugSamplerShape)]),
        "pl_debug_sample_positions": (cint, [cint, cint, cint, P(DebugSamplerMember), sz, P(C.c_uint32)]),
        "pl_debug_device_math": (cint, [cint, vp, sz, vp]),
        "pl_debug_device_math2": (cint, [cint, vp, vp, sz, vp]),
        "pl_refine_model": (cint, [vp, P(BundleOptions), cam, vp, vp, P(C.c_uint32)]),
        "pl_bundle_adjust_camera": (cint, [vp, P(BundleOptions), cam, vp, P(CameraPose), P(C.c_uint32)]),
        "pl_p3p": (cint, [vp, vp, P(CameraPose)]),
        "pl_relpose_5pt": (cint, [vp, vp, P(CameraPose)]),
        "pl_essential_matrix_5pt": (cint, [vp, vp, vp]),
        "pl_relpose_7pt": (cint, [vp, vp, vp]),
        "pl_homography_4pt": (cint, [vp, vp, vp]),
        "pl_solve_batch": (cint, [cint, vp, sz, vp, vp]),
    }
    missing = [name for name in EXPORTED_SYMBOLS if name not in sig]
    assert not missing, f"no signature declared for {missing}"
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    # the ctypes mirrors of this module restate the records of include/poselib_amd.h at PL_ABI_VERSION 5
    if L.pl_abi_version() != ABI_VERSION:
        raise PoseLibAmdError(f"{LIB_PATH} has record layout version {L.pl_abi_version()}, this binding was written for {ABI_VERSION}: rebuild")


def check(rc: int):
    if rc < 0:
        msg = lib().pl_last_error().decode()
        raise PoseLibAmdError(f"poselib_amd error {rc}: {msg}")
    return rc


ABI_VERSION = 5  # PL_ABI_VERSION of include/poselib_amd.h
EXPORTED_SYMBOLS = [
    "pl_default_ransac_options", "pl_default_bundle_options", "pl_default_robust_options", "pl_device_count",
    "pl_set_device", "pl_last_error", "pl_version", "pl_estimate_absolute_pose", "pl_estimate_relative_pose",
    "pl_estimate_fundamental", "pl_estimate_homography", "pl_ransac_pnp", "pl_ransac_relpose", "pl_ransac_fundamental",
    "pl_ransac_homography", "pl_problem_create", "pl_problem_destroy", "pl_ransac_run", "pl_ransac_run_sharded", "pl_score_model", "pl_debug_score_stream", "pl_refine_model", "pl_bundle_adjust_camera", "pl_p3p", "pl_relpose_5pt",
    "pl_essential_matrix_5pt", "pl_relpose_7pt", "pl_homography_4pt", "pl_solve_batch", "pl_estimate_batch", "pl_estimate_batch_devices", "pl_last_batch_report", "pl_undistort_points",
    "pl_ransac_batch", "pl_debug_device_math", "pl_debug_device_math2", "pl_ransac_pnpf", "pl_ransac_shared_focal_relpose", "pl_refine_shared_focal_relpose",
    "pl_estimate_shared_focal_relative_pose", "pl_solve_focal_batch", "pl_p35pf", "pl_relpose_6pt_shared_focal", "pl_set_lm_mode",
    "pl_abi_version", "pl_problem_create_tangent", "pl_debug_inlier_mask", "pl_debug_tangent_chunk",
    "pl_p5lp_radial", "pl_debug_radial1d_chunk", "pl_debug_radial1d_generate", "pl_debug_group_slices", "pl_debug_generate",
    "pl_debug_focal_stage",
    "pl_debug_score_shape", "pl_debug_score_stream_ex", "pl_debug_score_pruned", "pl_debug_score_survivors", "pl_debug_score_prune_gate",
    "pl_debug_score_bounded", "pl_debug_score_bounded_columns", "pl_debug_lm_route",
    "pl_estimate_absolute_pose_dev", "pl_estimate_relative_pose_dev", "pl_estimate_fundamental_dev", "pl_estimate_homography_dev",
    "pl_problem_create_dev", "pl_problem_create_tangent_dev", "pl_debug_check_device_points", "pl_debug_point_stats_dev",
    "pl_debug_sampler_shape", "pl_debug_sample_positions", "pl_estimate_batch_dev", "pl_debug_point_stats_group_dev",
    "pl_estimate_dev_scored", "pl_estimate_batch_dev_scored", "pl_debug_rank_scores", "pl_debug_rank_tile",
    "pl_undistort_points_dev", "pl_undistort_points_batch_dev", "pl_estimate_dev_masked", "pl_estimate_batch_dev_masked",
    "pl_estimate_shared_focal_relative_pose_dev", "pl_debug_point_stats_about_dev",
    "pl_estimate_shared_focal_relative_pose_batch_dev", "pl_debug_point_stats_about_group_dev",
    # (pl_estimate_1D_radial_absolute_pose, its _dev form and pl_ransac_1D_radial_pnp carry the reference's capital D: declared above, exported by the
    # library, but outside the lower-case pattern tests/test_cabi_surface.py lists the header's symbols with)
]
