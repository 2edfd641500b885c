"""poselib_amd — MI355X-native LO-RANSAC pose estimation, drop-in for the robust-estimation hot path of
PoseLib (estimate_absolute_pose / estimate_relative_pose / estimate_fundamental / estimate_homography,
ransac_*, and the p3p / relpose_5pt / relpose_7pt / homography_4pt minimal solvers).

All numerical work runs in hand-written HIP kernels (poselib_amd/csrc) behind the C-ABI declared in
include/poselib_amd.h; this package only marshals numpy arrays.  No CPU fallback.
"""
from ._lib import LIB_PATH, PoseLibAmdError, build  # noqa: F401
from .api import (  # noqa: F401
    KIND_ABS, KIND_FUND, KIND_HOM, KIND_REL, KIND_RAD1D, estimate_1D_radial_absolute_pose, ransac_1D_radial_pnp, p5lp_radial, radial1d_generate, debug_generate, debug_focal_stage, score_shape, score_stream_group, Batch, RansacBatch, ransac_batch, device_math, device_math2, BundleOptions, Camera, CameraPose, Image, Problem, TangentProblem, inlier_mask, RansacOptions,
    device_count, essential_matrix_5pt, estimate_absolute_pose, estimate_batch, last_batch_report, estimate_fundamental, estimate_homography,
    estimate_relative_pose, homography_4pt, p3p, p5p, ransac_fundamental, ransac_homography, ransac_pnp, ransac_pnpf,
    ransac_relpose, ransac_shared_focal_relpose, estimate_shared_focal_relative_pose, refine_shared_focal_relpose, ImagePair, p35pf, relpose_6pt_shared_focal, solve_focal_batch, relpose_5pt, relpose_7pt, set_device, set_lm_mode, solve_batch, undistort_points, undistort_points_batch,
    check_device_points, score_order, rank_scores, rank_tile, point_stats_dev, point_stats_group_dev, point_stats_about_dev, point_stats_about_group_dev, SharedFocalBatch, estimate_shared_focal_relative_pose_batch, score_pruned, score_survivors, score_bounded, score_prune_gate, lm_route, sampler_shape, sample_positions,
)

__version__ = "0.1.0"
