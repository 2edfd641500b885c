/* poselib_amd — C-ABI of the MI355X-native LO-RANSAC hot path.
 *
 * Drop-in boundary for the robust-estimation path of PoseLib 3.0.0 (citations relative to the
 * reference tree, PoseLib/...).  Every entry point is `extern "C"`, takes plain pointers and sizes
 * and is what a binding of the reference's API for this path would call:
 *
 *   pl_estimate_absolute_pose   <- robust.h:45-46     estimate_absolute_pose(points2D, points3D, opt, Image*, inliers*)
 *   pl_estimate_relative_pose   <- robust.h:68-70     estimate_relative_pose(x1, x2, camera1, camera2, opt, pose*, inliers*)
 *   pl_estimate_fundamental     <- robust.h:112-113   estimate_fundamental(x1, x2, opt, F*, inliers*)
 *   pl_estimate_homography      <- robust.h:133-134   estimate_homography(x1, x2, opt, H*, inliers*)
 *   pl_ransac_pnp / _relpose / _fundamental / _homography
 *                               <- robust/ransac.h:39-40, 60-61, 85-87, 99-101
 *   pl_p3p / pl_relpose_5pt / pl_essential_matrix_5pt / pl_relpose_7pt / pl_homography_4pt
 *                               <- solvers/p3p.h:42, relpose_5pt.h:40-43, relpose_7pt.h:39-40, homography_4pt.h:38-39
 *   pl_problem_* / pl_ransac_run <- the same ransac_* loop on correspondences that are already resident in
 *                                  HBM (what bench.py times), and its batched / multi-stream form.
 *
 * Conventions (identical to the reference's containers):
 *   - 2-D / 3-D points: contiguous AoS doubles, N x 2 / N x 3  (== std::vector<Eigen::Vector2d/3d>::data()).
 *   - pose: q[4] (w, x, y, z) then t[3];  3x3 matrices: COLUMN-major (== Eigen::Matrix3d::data()).
 *   - `inliers`: caller-allocated N bytes, 0/1 (the reference resizes a std::vector<char>).
 *   - in/out models are the initial model when ransac.score_initial_model != 0, otherwise they are
 *     overwritten (ransac.cc:47-50, 144-147, 252-254, 304-306).
 *   - Algorithmic "failure" is reported through the stats exactly like the reference (e.g. too few points
 *     => iterations == 0).  The int return value is 0 on success and a negative PL_ERR_* code for
 *     runtime failures only.  There is NO CPU fallback: without a usable HIP device every compute entry
 *     point returns PL_ERR_NO_DEVICE.
 *   - Thread-safety: re-entrant; each host thread gets its own HIP stream and scratch arena.
 */
#ifndef POSELIB_AMD_H_
#define POSELIB_AMD_H_
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PL_OK 0
#define PL_ERR_NO_DEVICE (-1)
#define PL_ERR_HIP (-2)
#define PL_ERR_INVALID (-3)
#define PL_ERR_UNSUPPORTED (-4)
#define PL_ERR_COMM (-5) /* the caller's all-gather callback failed (pl_ransac_run_sharded) */

/* types.h:39-50 */
typedef struct {
    uint64_t max_iterations;   /* 100000 */
    uint64_t min_iterations;   /* 1000 */
    double dyn_num_trials_mult; /* 3.0 */
    double success_prob;        /* 0.9999 */
    uint64_t seed;              /* 0 */
    int32_t progressive_sampling; /* PROSAC (sampling.cc:85-136): samples drawn on the host, models on the device */
    int32_t score_initial_model;
    uint64_t max_prosac_iterations;
} pl_ransac_options;

/* types.h:60-95 */
typedef struct {
    uint64_t max_iterations; /* 100 */
    int32_t loss_type;       /* 0 TRIVIAL, 1 TRUNCATED, 2 HUBER, 3 CAUCHY (default), 4 TRUNCATED_CAUCHY, 5 TRUNCATED_LE_ZACH */
    int32_t lambda_update;   /* 0 NIELSEN, 1 FIXED_FACTOR */
    int32_t damping;         /* 0 LEVENBERG, 1 MARQUARDT */
    int32_t verbose;         /* ignored */
    double loss_scale, gradient_tol, step_tol, relative_cost_tol, initial_lambda, min_lambda, max_lambda, lambda_factor;
    /* types.h:92-94.  Used by pl_estimate_absolute_pose's final bundle (robust.cc:103-123), its batched form and
     * pl_bundle_adjust_camera: the selected intrinsics of the camera move with the pose and are returned.  The two-view
     * refiners have no camera to move: ignored there, as in the reference. */
    int32_t refine_focal_length, refine_extra_params, refine_principal_point;
    int32_t reserved;
} pl_bundle_options;

/* types.h:108-126, 128-145, 170-175 folded into one record; fields that do not apply are ignored */
typedef struct {
    pl_ransac_options ransac;
    pl_bundle_options bundle;
    double max_error;         /* 12.0 absolute pose, 1.0 otherwise */
    int32_t real_focal_check; /* fundamental only */
    int32_t tangent_sampson;  /* pl_estimate_relative_pose (and relative-pose items of pl_estimate_batch): robust.cc:255-284 - the
                                 Sampson error is taken in the image, on unit bearings and the Jacobians of the un-projection
                                 (Terekhov & Larsson, CVPR 2023), for all nine camera models, with FIXED cameras: together with
                                 bundle.refine_focal_length / refine_principal_point / refine_extra_params the reference moves the
                                 intrinsics - that is PL_ERR_UNSUPPORTED.  Every other entry point: must be 0 */
    int32_t estimate_focal_length; /* pl_estimate_absolute_pose: robust.cc:47-54 - RANSAC over pose AND focal length (ransac_pnpf,
                                      P3.5Pf), the camera's focal length is replaced and refined in the final bundle; every
                                      other entry point: must be 0 */
    int32_t estimate_extra_params; /* must be 0 (radial distortion estimation: out of scope) */
    double min_fov;           /* types.h:126 AbsolutePoseOptions::min_fov, degrees (5.0): with estimate_focal_length / pl_ransac_pnpf the
                                 largest focal length a hypothesis may have is max|x| / tan(min_fov / 2) (absolute_pose.cc:159-177);
                                 <= 0 disables the bound; NaN is rejected (PL_ERR_INVALID).  Ignored by every other entry
                                 point, like in the reference.
                                 ABI note: this field was appended in PL_ABI_VERSION 4.  A caller must fill the record with
                                 pl_default_robust_options() and then change what it needs - a zero-initialised record
                                 means min_fov = 0 (NO bound) where the reference defaults to 5 degrees - and must be built
                                 against the header of the library it loads: check pl_abi_version() == PL_ABI_VERSION once. */
} pl_robust_options;

/* types.h:52-58 (+ the metric numerator and timing, which the reference does not report) */
typedef struct {
    uint64_t refinements, iterations, num_inliers;
    double inlier_ratio, model_score;
    uint64_t hypotheses;          /* minimal models scored against all N points in the main loop */
    uint64_t iterations_evaluated; /* iterations the device evaluated (>= iterations: speculative batches) */
    double seconds;                /* host wall time of the ransac_* part */
    double score_kernel_ms;        /* HIP-event time of the scoring kernel launches */
    uint32_t score_kernel_launches;
    uint32_t nan_hypotheses;       /* of the hypotheses the device evaluated: models with a NaN entry (the reference's
                                      P3P emits them for inconsistent samples; they have no inliers, utils.cc:36-65) */
} pl_ransac_stats;

/* misc/camera_models.h:56-60; supported ids: -1 NULL, 0 SIMPLE_PINHOLE {f cx cy}, 1 PINHOLE {fx fy cx cy},
 * 2 SIMPLE_RADIAL {f cx cy k1}, 3 RADIAL {f cx cy k1 k2}, 4 OPENCV {fx fy cx cy k1 k2 p1 p2},
 * 5 OPENCV_FISHEYE {fx fy cx cy k1 k2 k3 k4}, 8 SIMPLE_RADIAL_FISHEYE {f cx cy k}, 9 RADIAL_FISHEYE {f cx cy k1 k2} (the radius in
 * the image is f theta (1 + k1 theta^2 + k2 theta^4 ...), theta the angle to the optical axis); num_params at least the model's
 * count, for the fisheye models exactly the model's count (the reference's un-projection reads every parameter up to params.size()
 * as a coefficient of that polynomial, its projection the model's own: a longer list makes the two disagree).  Every other id
 * (FOV, THIN_PRISM_FISHEYE, division, FULL_OPENCV, thin-prism models, 1D_RADIAL, SPHERICAL) and a num_params that does not fit:
 * PL_ERR_UNSUPPORTED */
typedef struct {
    int32_t model_id, width, height, num_params;
    double params[12];
} pl_camera;

typedef struct {
    double q[4];
    double t[3];
} pl_camera_pose;

void pl_default_ransac_options(pl_ransac_options *o);
void pl_default_bundle_options(pl_bundle_options *o);
/* kind: 0 absolute pose (max_error 12), 1 relative pose, 2 fundamental, 3 homography (max_error 1), 5 absolute pose of a
 * 1D-radial camera (AbsolutePoseOptions: max_error 12); 4 is not a problem kind */
void pl_default_robust_options(pl_robust_options *o, int kind);

/* ---- device management ---- */
int pl_device_count(void);
int pl_set_device(int device);      /* device used by the calling thread from now on */
const char *pl_last_error(void);    /* thread-local description of the last failure */
const char *pl_version(void);
/* Layout version of the records in this header (bumped whenever a struct gains, loses or moves a field): 4 = round 4's
 * pl_robust_options.min_fov, 5 = round 5 (pl_set_lm_mode takes a mode 0 / 1 / 2, records unchanged).  A binding - C++, ctypes, cgo -
 * compares pl_abi_version() with the PL_ABI_VERSION it was written against before the first call that passes a record. */
#define PL_ABI_VERSION 5
int pl_abi_version(void);
/* Summation order of the non-linear refinements (optim/jacobian_accumulator.h:82-97 adds correspondence after correspondence).
 * 0 (default): poses and homographies - problems up to 256 correspondences are summed in the reference's order (refined models
 *    bit-identical), larger ones in tree order (refined models 1e-13 off; the decisions were identical in every test and soak);
 *    FUNDAMENTAL matrices - every sum in the reference's order at every size: FactorizedFundamentalMatrix (optim_utils.h:57-72)
 *    enters each refinement through an SVD and negates U / V by their determinants, so the SIGN of the F that is returned is the
 *    sign of a rounding-level singular value of the refinement's input - only bit-identical intermediate models give the
 *    reference's sign (1.8 x the refinement time at 10^4 correspondences with the truncated loss, none with Cauchy's).
 * 1: EVERY sum of every refinement in the reference's order at every size (k_lm_ordered) - refined models bit-identical at every
 *    n at 1.3 - 2 x the refinement time (6 x for homographies beyond 5000 correspondences).
 * 2: tree sums beyond 256 correspondences for every estimator, fundamental matrices included (their sign is then unpinned).
 * Process-wide; also POSELIB_AMD_LM_ORDERED = 0 / 1 / 2.  Returns the previous mode. */
int pl_set_lm_mode(int mode);

/* ---- robust front-ends (robust.h) ---- */
int pl_estimate_absolute_pose(const double *points2D, const double *points3D, size_t n, const pl_robust_options *opt,
                              pl_camera *camera, pl_camera_pose *pose, uint8_t *inliers, pl_ransac_stats *stats);
int pl_estimate_relative_pose(const double *points2D_1, const double *points2D_2, size_t n, const pl_camera *camera1,
                              const pl_camera *camera2, const pl_robust_options *opt, pl_camera_pose *pose,
                              uint8_t *inliers, pl_ransac_stats *stats);
/* robust.h:84-90 estimate_shared_focal_relative_pose (robust.cc:366-424): pixel coordinates, principal point pp[2]; the image pair
 * of the reference is (pose, SIMPLE_PINHOLE {focal, pp[0], pp[1]} for both cameras).  focal is read only with
 * ransac.score_initial_model (image_pair->camera1.focal()). */
int pl_estimate_shared_focal_relative_pose(const double *points2D_1, const double *points2D_2, size_t n, const double *pp,
                                           const pl_robust_options *opt, pl_camera_pose *pose, double *focal, uint8_t *inliers,
                                           pl_ransac_stats *stats);
int pl_estimate_fundamental(const double *points2D_1, const double *points2D_2, size_t n, const pl_robust_options *opt,
                            double *F /* 9, column-major */, uint8_t *inliers, pl_ransac_stats *stats);
int pl_estimate_homography(const double *points2D_1, const double *points2D_2, size_t n, const pl_robust_options *opt,
                           double *H /* 9, column-major */, uint8_t *inliers, pl_ransac_stats *stats);

/* ---- correspondences that are already in device memory (the output of a GPU matcher) ----
 * A point set as the _dev entry points below take it: rows of `cols` contiguous elements, float or double, `row_stride` ELEMENTS
 * apart - a contiguous N x cols block (row_stride == cols), a column view of a wider block, every k-th row of one.
 *   - The data must be COMPLETE when the call is made: the library works on a non-blocking stream of its own and takes no
 *     stream or event from the caller - synchronise the producer's stream first.
 *   - The data is read only during the call; pl_problem_create*_dev copy into the problem's own block before they return.
 *   - fp32 values are widened exactly, so a call equals the host call on the same values as doubles, bit for bit: model, mask
 *     and stats.
 *   - The memory must be DEVICE memory (hipMalloc and what builds on it) of the device the calling thread selected
 *     (pl_set_device), and the allocation must hold every row.  A host pointer, managed memory, memory of another device, a
 *     misaligned address, a row_stride below cols, another dtype or cols than the argument takes: PL_ERR_INVALID with a message
 *     that names the cause, before anything is launched.  n == 0 (and n below the estimator's minimum where the host form
 *     returns default stats) reads no device memory; data may then be null.
 * Models and stats stay in host memory; so do the `inliers` bytes of these entry points (pl_estimate_dev_masked, below, writes them
 * to device memory). */
#define PL_F64 0
#define PL_F32 1
typedef struct {
    const void *data;    /* device address of element (0, 0), on the device the calling thread selected */
    int64_t row_stride;  /* ELEMENTS between consecutive rows, >= cols; the columns of a row are contiguous */
    int32_t dtype;       /* PL_F64 / PL_F32 */
    int32_t cols;        /* 2 or 3: what the entry point expects for that argument */
} pl_device_points;
/* The host forms above with device-resident points; everything else as there.  pl_estimate_absolute_pose_dev with
 * estimate_focal_length: PL_ERR_UNSUPPORTED (that estimator reads the points on the host).  The batched form is
 * pl_estimate_batch_dev (below, behind pl_estimate_batch).  Not served from device memory: the focal-length estimators,
 * pl_estimate_1D_radial_absolute_pose, the pl_ransac_* one-shot entries. */
int pl_estimate_absolute_pose_dev(const pl_device_points *points2D, const pl_device_points *points3D, size_t n,
                                  const pl_robust_options *opt, pl_camera *camera, pl_camera_pose *pose, uint8_t *inliers,
                                  pl_ransac_stats *stats);
int pl_estimate_relative_pose_dev(const pl_device_points *points2D_1, const pl_device_points *points2D_2, size_t n,
                                  const pl_camera *camera1, const pl_camera *camera2, const pl_robust_options *opt,
                                  pl_camera_pose *pose, uint8_t *inliers, pl_ransac_stats *stats);
int pl_estimate_fundamental_dev(const pl_device_points *points2D_1, const pl_device_points *points2D_2, size_t n,
                                const pl_robust_options *opt, double *F /* 9, column-major */, uint8_t *inliers,
                                pl_ransac_stats *stats);
int pl_estimate_homography_dev(const pl_device_points *points2D_1, const pl_device_points *points2D_2, size_t n,
                               const pl_robust_options *opt, double *H /* 9, column-major */, uint8_t *inliers,
                               pl_ransac_stats *stats);
/* Every check the _dev entry points make on one argument that should hold n rows of `cols` columns, with their return code:
 * first the checks that need no device (null descriptor, null data with n > 0, cols, row_stride, dtype, alignment, n beyond
 * 2^31 - 1: PL_ERR_INVALID even on a machine without a GPU), then - n > 0 only - the memory's kind, device and extent. */
int pl_debug_check_device_points(const pl_device_points *d, size_t n, int cols);
/* Diagnostic: what the _dev front-ends read back from the device in place of the host's passes over the points, for two N x 2
 * sets.  out[8]: the centroids c1x c1y c2x c2y (the sums in index order, divided by n; zeros when `centroid` is 0), the scale of
 * the homography / fundamental normalisation (mean distance from the centroids in index order / sqrt(2)), the largest
 * |(x - c) / scale| over all four coordinates, the largest |coordinate| of the first set, and 0. */
int pl_debug_point_stats_dev(const pl_device_points *x1, const pl_device_points *x2, size_t n, int centroid, double *out);

/* ---- un-distortion as a stage of its own (BASELINE config 3: pixels of an OPENCV camera in front of the homography /
 * 7-point estimators, which take no camera).  Every point goes through Camera::unproject (misc/camera_models.h:98-102;
 * OPENCV: the iterative inverse of misc/camera_models.cc:972-990; SIMPLE_RADIAL / RADIAL: the Newton inverse of the radial
 * polynomial :579-611; the fisheye models: the Newton inverse of the polynomial in theta :613-662, then 1 / tan(theta)) and comes back as the pixel of the distortion-free
 * camera with the same focal lengths and principal point: out = (fx u + cx, fy v + cy).  points2D, out: N x 2.
 * camera: any supported model but NULL. ---- */
int pl_undistort_points(const pl_camera *camera, const double *points2D, size_t n, double *out);
/* The same stage for points that are in DEVICE memory and stay there (a tensor of distorted keypoints in front of the _dev
 * estimators): row i of `points2D` (fp32 or fp64, strided; fp32 widens exactly) is un-distorted into columns 0 and 1 of row i of
 * `out`, fp64, bit for bit what pl_undistort_points gives on the same values as doubles.  Nothing passes through the host.
 *   - camera: pl_undistort_points' rule (any supported model but NULL, otherwise PL_ERR_UNSUPPORTED).
 *   - points2D: the checks of every _dev entry point.  out: the same checks, and dtype PL_F64, cols 2, an 8-byte aligned address,
 *     row_stride >= 2, an allocation that holds every row.  The checks that need no device come first: PL_ERR_INVALID before
 *     PL_ERR_NO_DEVICE.  n == 0 reads and writes nothing; data may then be null.
 *   - Elements of a destination row beyond column 1 and rows beyond n are not written: columns of a wider block are a valid
 *     destination.
 *   - In place is allowed when the destination IS the source: same address, same row_stride, fp64.  Any other overlap of the two
 *     byte ranges (first byte of row 0 to last byte of row n - 1, whatever lies between the rows) is PL_ERR_INVALID.
 *   - The input must be complete when the call is made (synchronise the producer's stream first); the call returns after its own
 *     stream has been waited for, so the output is complete and visible to any stream.
 * Out of scope: fp32 output, a producer stream or event. */
typedef struct {
    void *data;          /* device address of element (0, 0), on the device the calling thread selected */
    int64_t row_stride;  /* ELEMENTS between consecutive rows, >= 2 */
    int32_t dtype;       /* PL_F64 only */
    int32_t cols;        /* 2 */
} pl_device_points_out;
int pl_undistort_points_dev(const pl_camera *camera, const pl_device_points *points2D, size_t n, const pl_device_points_out *out);
/* Many views at once - a matcher batch is 2 x pairs views over a handful of cameras; every item carries its own.  All descriptors
 * are checked first (an allocation's kind, device and extent are asked of the runtime once per allocation and call); a bad item
 * gets its own status and a message that names its index and the cause, the other items run: one argument table, one launch and
 * one synchronisation per call.  Every item equals its single call bit for bit.  Returns the first failing item's status. */
typedef struct {
    int32_t status;           /* out: PL_OK or the error of this item */
    int32_t reserved;         /* 0 */
    const pl_camera *camera;
    pl_device_points points2D;
    size_t n;
    pl_device_points_out out;
} pl_undistort_item_dev;
int pl_undistort_points_batch_dev(pl_undistort_item_dev *items, size_t count);

/* ---- batched front-end: an array of independent problems (BASELINE config 4: many image pairs) ----
 * Every item is one call of the matching pl_estimate_* above; `max_in_flight` problems (<= 0: 8) are worked on
 * concurrently by an internal pool of host threads, each with its own HIP stream and scratch arena, on the device the
 * calling thread selected with pl_set_device().  The reference has no such call: a PoseLib user loops over
 * estimate_*() (robust.h) from a thread pool, the Python wrappers release the GIL for that purpose. */
typedef struct {
    int32_t kind;            /* 0 absolute pose, 1 relative pose, 2 fundamental, 3 homography, 4 relative pose with a shared
                              * unknown focal length (pl_estimate_shared_focal_relative_pose).  Kind-4 items and kind-0 items with
                              * estimate_focal_length advance in lock-step groups of their own since round 5 (one launch sequence per
                              * group, every item bit-identical to its single call).  Kinds 0 - 3 with PROSAC, a warm start
                              * (ransac.score_initial_model) or a distorting camera (SIMPLE_RADIAL, RADIAL, OPENCV, the fisheye models) are group members like any other since round 6;
                              * what still runs one at a time: min_iterations > 4096, fewer correspondences than sample size + 4,
                              * more than 16384, warm starts of the focal-length kinds (pl_last_batch_report counts them) */
    int32_t status;          /* out: PL_OK or the error of this item */
    const double *a;         /* points2D (kind 0) / points2D_1: N x 2 */
    const double *b;         /* points3D: N x 3 (kind 0) / points2D_2: N x 2 */
    size_t n;
    const pl_robust_options *opt;
    pl_camera *camera1;      /* kind 0: in/out camera; kind 1: first camera; kind 4: SIMPLE_PINHOLE {focal, cx, cy} in/out; otherwise NULL */
    const pl_camera *camera2; /* kind 1: second camera; otherwise NULL */
    void *model;             /* in/out: pl_camera_pose (kinds 0, 1, 4) or double[9] column-major (kinds 2, 3) */
    uint8_t *inliers;        /* n bytes */
    pl_ransac_stats *stats;
} pl_batch_item;
/* returns PL_OK if every item succeeded, otherwise the status of the first failing item */
int pl_estimate_batch(pl_batch_item *items, size_t count, int max_in_flight);
/* The same call over SEVERAL devices of the node from one process (north_star: independent problems round-robined across the
 * GPUs; SURVEY 5 "one process drives <= 8 GPUs"): item i runs on devices[i mod num_devices], every entry of the list is served by
 * a host thread and a worker pool of its own (`max_in_flight` workers each), the results land in the caller's arrays - no
 * collective is needed inside one process.  devices == NULL or num_devices <= 0: every visible device.  An entry may repeat a
 * device (the list {0, 0} runs two half-batches side by side on device 0); every item is bit-identical to its single call
 * whatever the list.  The process-per-GPU form (one rank per device, RCCL gather of the result records) is the Python
 * harness's: poselib_amd/sharding.py, bench.py --gpus N; INTEGRATION.md says which to use when. */
int pl_estimate_batch_devices(pl_batch_item *items, size_t count, const int *devices, int num_devices, int max_in_flight);
/* pl_estimate_batch for correspondences that are already in DEVICE memory - the padded (pairs, N, 4) tensor of a GPU matcher, one
 * view per item.  The record is pl_batch_item with the two host pointers replaced by pl_device_points descriptors (by value);
 * every other field is unchanged, and model, inliers, stats, status, the options and the cameras stay in host memory.  The call
 * runs on the device the calling thread selected and keeps the contract of the single _dev calls: the data is complete when the
 * call is made and read only during it, fp32 widens exactly, and every item is bit-identical - model, mask, stats - to
 * pl_estimate_batch on the same values as doubles.  Several calls may be in flight from different host threads;
 * pl_last_batch_report reports the call like any other.
 *   - Every descriptor is checked before anything is launched (the checks of the single _dev calls; an allocation's kind, device
 *     and extent are asked of the runtime once per allocation and call, not per item).  A bad item gets status PL_ERR_INVALID
 *     and a message that names its index and the cause; the other items run; the call returns the first failing item's status.
 *     The checks that need no device come first: PL_ERR_INVALID before PL_ERR_NO_DEVICE.
 *   - Kinds 0 - 3 advance in lock-step groups under exactly pl_estimate_batch's conditions (PROSAC, warm starts and distorting
 *     cameras included).  The points of a group reach its kernels without passing through the host: one launch copies strided /
 *     fp32 members into the group's block (contiguous fp64 members are read where they lie), one launch makes the host
 *     front-ends' passes over the points of all members.  What a group does not take (too few or too many correspondences,
 *     min_iterations > 4096, tangent_sampson, items a group hands back) runs through the matching pl_estimate_*_dev and is
 *     counted solo / fallback.
 *   - Kind 4, kind 5 and kind 0 with estimate_focal_length: item status PL_ERR_UNSUPPORTED, as for the single calls; nothing is read.
 *   - Not offered: a form over several devices (the memory belongs to one), host and device items mixed in one call, a
 *     producer stream or event (synchronise the producer first).  Inlier masks in device memory: pl_estimate_batch_dev_masked.
 * Adding this record and entry point changes no existing record: PL_ABI_VERSION stays 5 (new symbols do not bump it). */
typedef struct {
    int32_t kind;            /* 0 absolute pose, 1 relative pose, 2 fundamental, 3 homography */
    int32_t status;          /* out: PL_OK or the error of this item */
    pl_device_points a;      /* points2D (kind 0) / points2D_1: N x 2 */
    pl_device_points b;      /* points3D: N x 3 (kind 0) / points2D_2: N x 2 */
    size_t n;
    const pl_robust_options *opt;
    pl_camera *camera1;      /* as pl_batch_item */
    const pl_camera *camera2;
    void *model;             /* in/out, host memory: pl_camera_pose (kinds 0, 1) or double[9] column-major (kinds 2, 3) */
    uint8_t *inliers;        /* n bytes, host memory */
    pl_ransac_stats *stats;
} pl_batch_item_dev;
int pl_estimate_batch_dev(pl_batch_item_dev *items, size_t count, int max_in_flight);
/* Diagnostic: pl_debug_point_stats_dev for `count` pairs of N x 2 sets at once, through the grouped kernels a group of
 * pl_estimate_batch_dev uses (one ingest launch, one statistics launch per pass, one synchronisation per pass).  x1, x2, n: count
 * entries each; out: count x 8 doubles, member after member, laid out as pl_debug_point_stats_dev's (zeros for n == 0). */
int pl_debug_point_stats_group_dev(const pl_device_points *x1, const pl_device_points *x2, const size_t *n, size_t count, int centroid,
                                   double *out);
/* ---- device-resident matches WITH their confidences: which rows are correspondences, and in which order (PROSAC) ----
 * A matcher leaves one confidence per row next to the matches and marks padding rows with a low (or NaN) one.  The _scored forms
 * of the _dev entry points take that output as it is.  THE RULE, for an item of n rows, scores s[0..n) and a threshold min_score:
 *   - row i is KEPT iff s[i] >= min_score (IEEE comparison): a NaN score is never kept.  min_score = -inf keeps every non-NaN
 *     row; -inf itself is kept only then; a NaN min_score is PL_ERR_INVALID;
 *   - kept rows are used in DESCENDING score (+inf first), equal scores in ASCENDING row index; -0.0 == 0.0;
 *   - in numpy: keep = s >= min_score; order = np.flatnonzero(keep)[np.argsort(-s[keep], kind="stable")].
 * (score, row) is a total order, so the permutation does not depend on how it is computed; fp32 scores widen exactly - a column
 * of floats ranks like the same values as doubles.  The estimator then runs EXACTLY as the plain entry point would on the rows
 * a[order], b[order] with n_used = len(order): the sampler's indices, the index-order sums of the normalisation, LM's summation
 * order and inlier_ratio (num_inliers / n_used) are those of that call, bit for bit.  inliers[i] speaks of the CALLER's row i
 * (n bytes; 0 for dropped rows).  Whatever the plain form serves or refuses for n_used rows, the scored form serves or refuses
 * the same way (too few rows: default stats; tangent_sampson; estimate_focal_length: PL_ERR_UNSUPPORTED).
 * Scores reorder and select - they do NOT switch PROSAC on: ransac.progressive_sampling selects the sampler, as everywhere.
 *   - The scores get the checks the points get, in the same order (null descriptor, n beyond 2^31 - 1, dtype, stride < 1, null
 *     data, alignment - PL_ERR_INVALID without a device -, then the memory's kind, device and extent).  They are read only
 *     during the call and must be complete when it is made.
 *   - How: a ranking kernel leaves the permutation and the kept count in device memory, a permuting copy (the ingest kernel
 *     reading row order[j] into row j) writes the contiguous fp64 blocks the preparation takes - a scored item is never read where
 *     it lies -, one synchronisation brings count and permutation back; the mask is scattered to the caller's numbering on the
 *     host (on the device, without a copy, by the _masked forms below).  Any n up to 2^31 - 1; the work buffers are 24 bytes per
 *     row beyond 8192 rows, none below.
 *   - Out of scope: models in device memory, a producer stream, scored resident problems (pl_problem_create_dev),
 *     scores for estimate_focal_length and the pl_ransac_* entries, half-precision scores.  (The shared-focal and 1D-radial
 *     estimators take scores through their own _dev entry points, below.) */
typedef struct {
    const void *data;   /* device address of the first row's score */
    int64_t stride;     /* ELEMENTS between consecutive rows' scores, >= 1: one column of a wider block is a valid source */
    int32_t dtype;      /* PL_F64 / PL_F32 */
    int32_t reserved;   /* 0 */
    double min_score;   /* rows with score >= min_score are kept; -INFINITY keeps every non-NaN row */
} pl_device_scores;
/* kind 0 .. 3 as pl_batch_item_dev.kind; camera1 / camera2 / model as there (kind 0: camera1 in/out, pose; kind 1: both cameras,
 * pose; kinds 2, 3: no cameras, double[9] column-major).  n_used (optional): the kept count. */
int pl_estimate_dev_scored(int kind, const pl_device_points *a, const pl_device_points *b, const pl_device_scores *scores, size_t n,
                           const pl_robust_options *opt, pl_camera *camera1, const pl_camera *camera2, void *model, uint8_t *inliers,
                           pl_ransac_stats *stats, size_t *n_used);
/* pl_estimate_batch_dev with scores: scores[i] belongs to items[i]; an entry whose data is NULL makes item i a plain item (scores
 * == NULL: every item).  ALL scored items are ranked first - one launch sequence and one synchronisation per call, not per item -
 * and the groups are then formed on n_used: an item is a group member when sample size + 4 <= n_used <= 16384, whatever its n.
 * Every item equals its single call bit for bit, pl_last_batch_report reports the call like any other, and a bad scores
 * descriptor fails its own item only (PL_ERR_INVALID, the message names index and cause).  n_used (optional): count entries,
 * items[i].n for a plain item, 0 for an item that did not run. */
int pl_estimate_batch_dev_scored(pl_batch_item_dev *items, const pl_device_scores *scores, size_t *n_used, size_t count,
                                 int max_in_flight);
/* ---- inlier masks written to DEVICE memory: what one does next with a mask is index the match tensor, so it need not come down ----
 * A mask destination, parallel to pl_device_scores.  THE RULE, for an item of n rows: byte i * stride of the destination becomes 0
 * or 1 for every i in [0, n) - all n of them, always - with the values of the host mask of the same call made on a buffer that was
 * zero-filled beforehand: rows dropped by the scores give 0, and where the host form writes nothing (too few rows, an item that
 * failed after its descriptors were accepted) all n bytes are 0.  No other byte is touched.  Model, stats, n_used, the status and
 * pl_last_batch_report are bit for bit what the call with a host mask gives.
 *   - The destination gets the points' checks (null descriptor, n beyond 2^31 - 1, stride < 1, null data - PL_ERR_INVALID without
 *     a device -, then the memory's kind, device and extent); a bad descriptor fails its own item, whose destination is not touched.
 *   - The destination must not overlap the points or the scores: that is the CALLER's contract, it is not checked.
 *   - How: one launch zero-fills every destination of the call; the launch that computes the returned model's mask - of the
 *     item's lock-step group, or of its single run (solo, fallback and deferred items take that route as well) - writes the flags
 *     into the destination itself, a scored item's through the permutation its ranking left in device memory.  Such an item has
 *     no pinned host mask, no device-to-host copy and no scatter on the host.  The call returns after its streams have been
 *     waited for: the mask is complete and visible to any stream.
 *   - Out of scope: models or stats in device memory (the front-ends finish the model on the host), a producer stream or event,
 *     masks for resident problems (pl_problem_create_dev) and the pl_ransac_* entries, anything for kinds 4 and 5 of the batch
 *     and the kind-numbered entry points and for estimate_focal_length, whose refusals stay as they are (single calls of the
 *     shared-focal and 1D-radial estimators: their own _dev entry points, below). */
typedef struct {
    uint8_t *data;      /* device address of row 0's flag */
    int64_t stride;     /* BYTES between consecutive rows' flags, >= 1: a bool / uint8 tensor, or one column of a wider byte block */
} pl_device_mask;
/* pl_estimate_dev_scored (scores != NULL) or the plain _dev entry point of `kind` (scores == NULL) with the mask in device memory. */
int pl_estimate_dev_masked(int kind, const pl_device_points *a, const pl_device_points *b, const pl_device_scores *scores /* may be NULL */,
                           size_t n, const pl_robust_options *opt, pl_camera *camera1, const pl_camera *camera2, void *model,
                           const pl_device_mask *mask, pl_ransac_stats *stats, size_t *n_used);
/* pl_estimate_batch_dev_scored with masks[i] belonging to items[i]: an entry whose data is NULL makes item i an item with its host
 * `inliers` pointer as ever (masks == NULL: every item); items[i].inliers is ignored when a device mask is given. */
int pl_estimate_batch_dev_masked(pl_batch_item_dev *items, const pl_device_scores *scores /* may be NULL */, const pl_device_mask *masks,
                                 size_t *n_used, size_t count, int max_in_flight);
/* Diagnostic: the permutation alone.  scores, n, kept: count entries; order: the members one after the other, n[k] slots each, the
 * first kept[k] of them written.  count == 1 takes the kernels' single form, count > 1 the grouped one (one launch sequence for
 * all members).  pl_debug_rank_tile: the rows one workgroup ranks out of LDS in a launch whose largest member has max_n rows -
 * members up to it need one launch, larger ones merge passes through global memory. */
int pl_debug_rank_scores(const pl_device_scores *scores, const size_t *n, size_t count, uint32_t *order, size_t *kept);
int pl_debug_rank_tile(size_t max_n);
/* ---- the two estimators of UNKNOWN cameras from device memory: shared focal length (two views of one uncalibrated camera) and
 * 1D-radial absolute pose (unknown distortion).  One entry point each covers the plain, the scored and the device-mask form:
 *   scores (may be NULL)  THE RULE of pl_device_scores: the call is the host entry point's on a[order], b[order], the mask speaks of
 *                         the caller's rows, n_used = len(order) (n without scores).  The index-order sums in front of the loop -
 *                         the mean distance from pp; n / sum |x_k| - are taken over the ranked rows in ranked order.
 *   mask (may be NULL)    pl_device_mask's rule: all n bytes are written, dropped rows and a call whose host form writes no mask give
 *                         0; `inliers` is then ignored, there is no pinned host mask and no scatter on the host.
 *   inliers (host, may be NULL), stats, n_used (may be NULL)  as everywhere.
 * The result - pose, focal length, mask and every field of the stats except `seconds` - is the host entry point's
 * (pl_estimate_shared_focal_relative_pose, pl_estimate_1D_radial_absolute_pose) on the same values, bit for bit; float32 widens
 * exactly.  What the host form answers without a launch is answered the same way before any launch: the option validation, null pp /
 * pose / focal (PL_ERR_INVALID), 1D-radial with n < 5 (default stats, pose untouched; with scores or a device mask the device is
 * asked first: n_used and the mask's zeros need it).  The descriptors get the points' checks without a device (PL_ERR_INVALID),
 * then the memory's kind, device and extent.
 *   - How: the rows become contiguous fp64 blocks on the device (read where they lie when they already are; the ranking's
 *     permuting copy for a scored call); one single-workgroup launch adds the host's sum in the host's order and returns one small
 *     record; shared focal then prepares the problem from those blocks, 1D radial writes its block of scaled pixels with the
 *     ingest kernel - and from there the host forms' own code runs.  No point passes through the host.
 *   - Out of scope: these two in pl_estimate_batch_dev (kinds 4 and 5 stay refused there; batches of shared-focal pairs:
 *     pl_estimate_shared_focal_relative_pose_batch_dev below), estimate_focal_length. */
int pl_estimate_shared_focal_relative_pose_dev(const pl_device_points *x1, const pl_device_points *x2,
                                               const pl_device_scores *scores /* may be NULL */, size_t n, const double *pp,
                                               const pl_robust_options *opt, pl_camera_pose *pose, double *focal,
                                               uint8_t *inliers /* host, may be NULL */,
                                               const pl_device_mask *mask /* may be NULL; then inliers is ignored */,
                                               pl_ransac_stats *stats, size_t *n_used /* may be NULL */);
int pl_estimate_1D_radial_absolute_pose_dev(const pl_device_points *points2D, const pl_device_points *points3D,
                                            const pl_device_scores *scores /* may be NULL */, size_t n, const pl_robust_options *opt,
                                            pl_camera_pose *pose, uint8_t *inliers /* host, may be NULL */,
                                            const pl_device_mask *mask /* may be NULL; then inliers is ignored */, pl_ransac_stats *stats,
                                            size_t *n_used /* may be NULL */);
/* Diagnostic: the two reductions alone.  x2 != NULL: the mean distance of both sets from (cx, cy), correspondence after
 * correspondence, over sqrt(2) * n (shared focal); x2 == NULL: n / sum_k sqrt(0.0 + x_k^2 + y_k^2) of x1 in index order (1D
 * radial; cx, cy unused).  out[0] = the scale, out[1] = max |coordinate * scale| (radial; a NaN propagates) or 0. */
int pl_debug_point_stats_about_dev(const pl_device_points *x1, const pl_device_points *x2 /* NULL: radial */, size_t n, double cx,
                                   double cy, double *out /* 2 */);
/* ---- batches of shared-focal pairs from device memory: what a matcher's padded (pairs, N, 5) tensor holds, in one call.
 * pl_estimate_batch_dev* and the kind-numbered _dev entries keep refusing kind 4; this entry point of its own serves it.
 *   - Every item is pl_estimate_shared_focal_relative_pose_dev on the same arguments, bit for bit (and so the host call on the
 *     same values as doubles): pose, focal length, the mask in the caller's row numbering, n_used and every field of the stats
 *     except `seconds`.  A result does not depend on the item's group, on max_in_flight or on POSELIB_AMD_FOCAL_GROUP.
 *   - scores / masks: NULL, or count entries belonging to items[i]; an entry whose data is NULL makes item i a plain item / an
 *     item with its host `inliers` pointer (which is ignored when a device mask is given).  n_used: NULL, or count entries.
 *   - All descriptors are checked before any launch, the checks that need no device first (PL_ERR_INVALID comes before
 *     PL_ERR_NO_DEVICE), then the memory's kind, device and extent - the runtime is asked once per allocation and call.  A bad
 *     item, or one with a null opt / pose / focal or options the single call rejects, fails alone with the status its single call
 *     would give and the message "item k: cause"; its mask destination is not touched; the other items run; the call returns
 *     the first failing item's status.  count == 0: PL_OK; items == NULL with count > 0: PL_ERR_INVALID.
 *   - How: one zero-fill launch over all device masks first; all scored items ranked at once (one launch sequence, one
 *     synchronisation); then the items the lock-step groups of pl_estimate_batch's kind 4 take - judged on n_used:
 *     10 <= n_used <= 16384, no warm start, max_iterations > 0, min_iterations <= 4096, PROSAC included - advance in groups whose
 *     first stage reads the rows where they lie: strided / fp32 members are copied into the group's block, one launch adds every
 *     member's mean distance from its pp in index order, and the normalisation launch behind it takes each scale from the member's
 *     record on the device - no point and no scale passes through the host in between.  A member's mask launch writes a device
 *     mask itself, a scored member's through its ranking's permutation.  Everything else, and items a group hands back, runs through the
 *     single _dev entry point (a scored one on its ranked blocks).  pl_last_batch_report: items, focal_grouped, solo, fallback
 *     (grouped is 0).  Several calls may be in flight from different host threads.
 *   - Out of scope: several devices, host and device items mixed in one call, a producer stream, models in device memory,
 *     1D-radial batches and estimate_focal_length from device memory.
 * Adding this record and entry point changes no existing record: PL_ABI_VERSION stays 5 (new symbols do not bump it). */
typedef struct {
    int32_t status;              /* out */
    int32_t reserved;            /* 0 */
    pl_device_points x1, x2;     /* N x 2 each */
    size_t n;
    double pp[2];
    const pl_robust_options *opt;
    pl_camera_pose *pose;        /* host, in/out as in the single call */
    double *focal;               /* host, in/out as in the single call */
    uint8_t *inliers;            /* host, n bytes, may be NULL */
    pl_ransac_stats *stats;      /* may be NULL */
} pl_shared_focal_item_dev;
int pl_estimate_shared_focal_relative_pose_batch_dev(pl_shared_focal_item_dev *items,
                                                     const pl_device_scores *scores /* may be NULL; an entry without data: a plain item */,
                                                     const pl_device_mask *masks /* may be NULL; an entry without data: host mask */,
                                                     size_t *n_used /* may be NULL */, size_t count, int max_in_flight);
/* Diagnostic: the reduction in front of that call's groups alone - pl_debug_point_stats_about_dev (x2 != NULL) for count pairs at
 * once through the grouped kernels, every member about its own centre (centres: count x 2).  out: count x 2, {scale, 0} per member. */
int pl_debug_point_stats_about_group_dev(const pl_device_points *x1, const pl_device_points *x2, const size_t *n, const double *centres,
                                         size_t count, double *out /* count x 2 */);
/* What the calling thread's last pl_estimate_batch / pl_estimate_batch_devices / pl_estimate_batch_dev /
 * pl_estimate_shared_focal_relative_pose_batch_dev / pl_ransac_batch did with its items.  Items in
 * lock-step groups share one launch sequence (the advertised rate); `solo` items were outside the group path from the start
 * (options or sizes a group does not take - see pl_batch_item / pl_ransac_batch) and `fallback` items were handed back by their
 * group: both kinds ran through the single-problem entry points, correct but at that path's rate - a batch that is mostly solo
 * items runs ~20 x slower than one that is grouped, and this report is where a caller sees it. */
typedef struct {
    uint64_t items;         /* items of the call */
    uint64_t grouped;       /* ... in the lock-step groups of kinds 0 - 3 */
    uint64_t focal_grouped; /* ... in the groups of the two focal-length estimators */
    uint64_t solo;          /* ... run one at a time from the start */
    uint64_t fallback;      /* of the grouped ones: handed back by their group and re-run one at a time */
} pl_batch_report;
void pl_last_batch_report(pl_batch_report *out);

/* ---- RANSAC entry points on normalised points (robust/ransac.h) ---- */
int pl_ransac_pnp(const double *x, const double *X, size_t n, const pl_robust_options *opt, pl_camera_pose *pose,
                  uint8_t *inliers, pl_ransac_stats *stats);
/* robust/ransac.h:52-54 ransac_pnpf (FocalAbsolutePoseEstimator, estimators/absolute_pose.h:69-113): pose and focal length of a
 * SIMPLE_PINHOLE camera whose principal point is the origin of the image points x.  The model is reset before the loop as in
 * the reference (ransac.cc:61-66); opt->min_fov bounds the focal length (absolute_pose.h:78).  PROSAC sampling: samples drawn on the host. */
int pl_ransac_pnpf(const double *x, const double *X, size_t n, const pl_robust_options *opt, pl_camera_pose *pose, double *focal,
                   uint8_t *inliers, pl_ransac_stats *stats);
int pl_ransac_relpose(const double *x1, const double *x2, size_t n, const pl_robust_options *opt, pl_camera_pose *pose,
                      uint8_t *inliers, pl_ransac_stats *stats);
/* robust/ransac.h:71-73 ransac_shared_focal_relpose (SharedFocalRelativePoseEstimator, estimators/relative_pose.h:148-175; solver:
 * the 6-point shared-focal problem of solvers/relpose_6pt_focal.h): relative pose of two views of ONE camera with unknown focal
 * length; x1, x2 relative to the principal point.  pose / focal: the initial model when ransac.score_initial_model is set (otherwise
 * reset as in ransac.cc:185-190), the result on return.  PROSAC sampling (sampling.cc:85-136): samples drawn on the host, as for pl_ransac_pnpf. */
int pl_ransac_shared_focal_relpose(const double *x1, const double *x2, size_t n, const pl_robust_options *opt, pl_camera_pose *pose,
                                   double *focal, uint8_t *inliers, pl_ransac_stats *stats);
/* robust/bundle.h:108-111 refine_shared_focal_relpose (SharedFocalRelativePoseRefiner, optim/relative.h:488-592): pose and the
 * shared focal length refined on all n correspondences (Sampson error of F = K^-1 E K^-1); both in / out. */
int pl_refine_shared_focal_relpose(const double *x1, const double *x2, size_t n, const pl_bundle_options *opt, pl_camera_pose *pose,
                                   double *focal, uint32_t *lm_iterations);

int pl_ransac_fundamental(const double *x1, const double *x2, size_t n, const pl_robust_options *opt, double *F,
                          uint8_t *inliers, pl_ransac_stats *stats);
int pl_ransac_homography(const double *x1, const double *x2, size_t n, const pl_robust_options *opt, double *H,
                         uint8_t *inliers, pl_ransac_stats *stats);
/* Absolute pose of a camera with unknown (or unmodelled) radial distortion - the reference's 1D-radial camera: no intrinsics,
 * points2D are pixels relative to the centre of distortion (N x 2), points3D N x 3.  The pose has t[2] = 0: the error - the
 * distance of a pixel from the radial line through its point's projection, on the projection's side of the centre - does not
 * see the forward translation.
 * pl_estimate_1D_radial_absolute_pose (robust.cc:889-934): the pixels, max_error and bundle.loss_scale are rescaled by the mean
 * pixel norm, RANSAC on the radial 5-point solver (p5lp_radial) with local optimisation, then bundle_adjust_1D_radial over the
 * inliers when there are more than 5.  n < 5: default stats, pose and inliers untouched.  bundle.refine_* has no effect.
 * pl_ransac_1D_radial_pnp (ransac.cc:388-401): the RANSAC stage alone, nothing rescaled.
 * The 1D-radial camera model inside the OTHER estimators (a pl_camera with that model id) stays unsupported. */
int pl_estimate_1D_radial_absolute_pose(const double *points2D, const double *points3D, size_t n, const pl_robust_options *opt,
                                        pl_camera_pose *pose, uint8_t *inliers, pl_ransac_stats *stats);
int pl_ransac_1D_radial_pnp(const double *x, const double *X, size_t n, const pl_robust_options *opt, pl_camera_pose *pose,
                            uint8_t *inliers, pl_ransac_stats *stats);

/* ---- device-resident problems (inputs stay in HBM across calls; what bench.py times) ---- */
typedef struct pl_problem pl_problem;
/* kind as in pl_default_robust_options; a = first point set (N x 2), b = second (N x 3 for kinds 0 and 5, else N x 2).  Kind 5
 * (1D-radial absolute pose): a = centred pixels as pl_ransac_1D_radial_pnp takes them; models are pl_camera_pose; pl_refine_model is
 * bundle_adjust_1D_radial; pl_ransac_run_sharded answers PL_ERR_UNSUPPORTED for it */
int pl_problem_create(int kind, const double *a, const double *b, size_t n, pl_problem **out);
/* A resident tangent-Sampson relative-pose problem: per correspondence the bearings of the two pixels and the 3x2 Jacobians of
 * the un-projections (Camera::unproject_with_jac), computed on the device.  x1 / x2 (N x 2 pixels) and the cameras are taken as
 * they stand: the level of ransac_relpose(x1, x2, camera1, camera2, ...), behind estimate_relative_pose's rescaling.  A null
 * camera is the identity camera.  Models are pl_camera_pose. */
int pl_problem_create_tangent(const double *x1, const double *x2, size_t n, const pl_camera *camera1, const pl_camera *camera2,
                              pl_problem **out);
/* pl_problem_create (kinds 0 - 3 and 5) and pl_problem_create_tangent from device-resident points (pl_device_points above): the
 * problem's block is written on the device, nothing passes through the host, and the problem equals the one the host form
 * builds from the same values.  Such problems go into pl_ransac_run / pl_ransac_batch like any other. */
int pl_problem_create_dev(int kind, const pl_device_points *a, const pl_device_points *b, size_t n, pl_problem **out);
int pl_problem_create_tangent_dev(const pl_device_points *x1, const pl_device_points *x2, size_t n, const pl_camera *camera1,
                                  const pl_camera *camera2, pl_problem **out);
void pl_problem_destroy(pl_problem *p);
/* model: pl_camera_pose for kinds 0/1, double[9] column-major for kinds 2/3 */
int pl_ransac_run(pl_problem *p, const pl_robust_options *opt, void *model, uint8_t *inliers, pl_ransac_stats *stats);

/* ---- many device-resident problems at once: every item is one pl_ransac_run (a loop over ransac_pnp / ransac_relpose /
 * ransac_fundamental / ransac_homography of robust/ransac.h:45-66 on the reference side), same results bit for bit.
 * Items of the same kind advance in lock-step groups of `group_size` problems (<= 0: 16, at most 64): one launch sequence
 * per group and batch of iterations instead of one per problem, which is what keeps the device busy when thousands of
 * problems are queued (bench.py's throughput mode).  `max_in_flight` host threads (<= 0: 4), each with its own stream,
 * work on different groups.  Items a group cannot take (fewer correspondences than sample size + 4, more than 16384) run
 * through pl_ransac_run; PROSAC and warm starts are group members since round 6.  The problems may live on DIFFERENT devices (pl_set_device before
 * pl_problem_create): every item runs on the device that holds its problem, one host thread and one worker pool per device
 * side by side (round 6). ---- */
typedef struct {
    pl_problem *problem;
    const pl_robust_options *opt;
    void *model;            /* out: pl_camera_pose (kinds 0, 1) or double[9] column-major (kinds 2, 3); in as well when
                               opt->ransac.score_initial_model is set */
    uint8_t *inliers;       /* optional, problem size bytes */
    pl_ransac_stats *stats; /* optional */
    int32_t status;         /* out: PL_OK or the error of this item */
    int32_t reserved;
} pl_ransac_item;
int pl_ransac_batch(pl_ransac_item *items, size_t count, int max_in_flight, int group_size);

/* ---- ONE problem across several GPUs: every rank holds the same correspondences (its own pl_problem on
 * its own device) and calls pl_ransac_run_sharded with the same options.  Each batch of iterations is cut into `world`
 * contiguous ranges; a rank draws the whole batch's sample positions (integer work, replicated) but generates and
 * scores only its range.  Two exchange steps per batch: the ranks all-gather their improving hypotheses (<= 7 KB per
 * rank, another message only when a rank has more than 32 of them), deal the triggered local optimisations out
 * among themselves (job j on rank j mod world) and all-gather the refined models (0.2 KB per job); every rank then
 * replays the sequential loop of ransac_impl.h:157-201 on the merged data, so all ranks return the same model, mask
 * and stats, identical to the single-device run.  `allgather` is the caller's
 * collective (RCCL / gloo through torch.distributed, MPI, or shared memory between threads): it must copy `bytes` bytes
 * from `send` of rank r to `recv + r * bytes` on every rank, and return 0. */
typedef int (*pl_allgather_fn)(void *user, const void *send, void *recv, size_t bytes);
typedef struct pl_shard {
    int32_t rank, world;
    pl_allgather_fn allgather;
    void *user;
} pl_shard;
int pl_ransac_run_sharded(pl_problem *p, const pl_robust_options *opt, const pl_shard *shard, void *model,
                          uint8_t *inliers, pl_ransac_stats *stats);

/* Score one model against the resident correspondences with the estimator's MSAC score
 * (robust/utils.cc:36-65, 158-239, 300-329 through estimators' score_model()).  model as in pl_ransac_run. */
int pl_score_model(pl_problem *p, const void *model, double max_error, uint64_t *inlier_count, double *score);
/* Diagnostic: the inlier mask (N bytes) of one model, as the estimators' final inlier pass computes it. */
int pl_debug_inlier_mask(pl_problem *p, const void *model, double max_error, uint8_t *mask);
/* Diagnostic: correspondences per chunk of the tangent-Sampson streaming scorer as built. */
int pl_debug_tangent_chunk(void);
/* ... and of the 1D-radial streaming scorer */
int pl_debug_radial1d_chunk(void);
/* Diagnostic: the hypothesis slices per chunk of correspondences that the scorer launch of a lock-step group (pl_ransac_batch,
 * pl_estimate_batch) gives ONE member - a problem of `kind` (0, 1, 2, 3 or 5) with n_points correspondences and a batch of
 * `iterations` iterations - when the chunks of correspondences of all active members of the launch, this one included, add up
 * to launch_chunks (a smaller value counts as the member alone).  Whether a real member is scored on the matrix cores also
 * depends on its coordinates and threshold; this entry assumes both in the pre-filters' range, so the kind, the size and
 * POSELIB_AMD_NO_MFMA decide.  Absolute pose on the matrix cores (n_points >= 1024) takes
 * fewer slices the more the launch holds; every other scorer does not depend on launch_chunks.  Host arithmetic only: no device
 * is touched.  Returns the count (>= 1), or PL_ERR_INVALID. */
int pl_debug_group_slices(int kind, uint32_t n_points, uint32_t iterations, uint32_t launch_chunks);
/* Diagnostic: the generator kernel of a resident kind-5 problem on caller-supplied minimal samples (num_iters x 5 indices - the path
 * PROSAC's host-drawn samples take) with slots_per_iter (1 .. 4) record slots per iteration.  models: num_iters x slots_per_iter
 * records of 24 doubles (zero where none was written); num_models: num_iters; totals[3]: models counted, models with a NaN entry,
 * overflow flag (an iteration had more solutions than slots: its count is 0). */
int pl_debug_radial1d_generate(pl_problem *p, const uint32_t *samples, size_t num_iters, uint32_t slots_per_iter, double *models,
                               uint32_t *num_models, uint32_t *totals);
/* Diagnostic: the hypothesis generator of the main loop on its own - the kernels a batch step launches, wired as a batch step wires
 * them - for a resident problem of kind 0, 1, 2, 3 or 5 or a tangent problem, with every iteration's output copied back.  tests/
 * compares them with the reference estimators' generate_models hypothesis by hypothesis.
 * Samples: either `samples` (num_iters x K indices, K = the kind's minimal sample; each must be < the problem's size) or `positions`
 * (num_iters entries: draws consumed before each iteration, relative to pos_base) with `seed` for the device's own sampler; exactly one
 * of the two is non-NULL.  slots_per_iter: record slots per iteration, 1 .. the kind's maximum (4, 40, 3, 1; kind 5: 4); an iteration
 * with more solutions sets the overflow flag and counts 0.  real_focal_check: kind 2 only.
 * route 0: the single-problem launch (kind 1 and tangent problems: the staged 5-point generator); 1: the single-kernel 5-point
 * generator (kind 1 only); 2: the group form (kinds 0 - 3) over a table of three slots - slot 0 inactive, slot 1 this problem with all
 * num_iters iterations, slot 2 this problem with its first ceil(num_iters / 3) iterations and output buffers of its own - launched for
 * num_iters iterations.  Routes 0 and 1 have one member, route 2 two (slots 1 and 2); member m's outputs follow member m - 1's:
 *   models     members x num_iters x slots_per_iter records of 24 doubles, zeroed before the launch
 *   num_models members x num_iters, 0xffffffff before the launch
 *   nan_bits   members x num_iters, may be NULL, written for kind 0 only (bit m: record m holds a NaN), 0xffffffff before the launch
 *   blk_tot, blk_nan  members x ceil(num_iters / 1024): models and NaN models per block of 1024 iterations as the generator counted them
 *   flags[3]   overflow flag of member 0, of member 1, and (route 2) the number of words the inactive slot's buffers changed in.
 * PL_ERR_INVALID: num_iters 0 or above 2^20, slots_per_iter out of range, an index beyond the problem, fewer correspondences than K with
 * `positions`, route 1 for another kind than 1, route 2 for a tangent or kind-5 problem. */
int pl_debug_generate(pl_problem *p, const uint32_t *samples, uint64_t seed, uint64_t pos_base, const uint32_t *positions, size_t num_iters,
                      uint32_t slots_per_iter, int real_focal_check, int route, double *models, uint32_t *num_models, uint32_t *nan_bits,
                      uint32_t *blk_tot, uint32_t *blk_nan, uint32_t *flags);
/* Diagnostic: ONE stage of the two focal-length estimators on its own - the generator (k_focal_setup + k_focal_solve /
 * k_sfocal_setup + k_sfocal_solve), the scorers (k_focal_score[_wg] / k_sfocal_score[_wg]) or the mask kernel - through the
 * production launchers, with the arguments wired as the estimators' back ends wire them (models, counts and the workspace in device
 * memory; the mirrors, the scores and the LM task records in pinned mapped memory).  Problems of kind 0 run the kernels of
 * ransac_pnpf, problems of kind 2 those of ransac_shared_focal_relpose; every member of one call has the same kind.
 * stage 0 generate, 1 score, 2 mask.  group 0: one member through the single-problem launcher (the score launcher's own rule picks the
 * kernel: one workgroup per model up to 1024 slots, one wavefront per model - with num_models on kind 2, one workgroup per iteration -
 * above); group 1: 1 .. 8 members as a device-resident table through the group launcher, whose grid is the largest member's;
 * workgroup_per_model selects the group score kernel (0 on kind 2 requires num_models: the launcher's grid is one workgroup per
 * iteration).  A member:
 *   problem, idle   idle 1: wired with n = 0 and no iterations / slots / correspondences over real buffers - nothing may be written
 *   count           generate: iterations (1 .. 2^20); score: slots (1 .. 2^20); mask: unused (the problem's n)
 *   capacity        extent of the member's output buffers in the same unit (mask: bytes, >= n), >= count; what lies beyond the
 *                   member's own extent must keep the prefill
 *   generate        samples (count x 4 | 6 indices < n) or positions (count draws, relative to pos_base, with seed) - exactly one;
 *                   max_focal (kind 0; < 0: no bound).  Outputs: out_models capacity x (10 | 60) x 8 doubles (q, t, f) and
 *                   out_num_models capacity from device memory, out_host_models / out_host_num_models the pinned mirrors
 *   score           models count x 8 doubles; num_models (optional gate: count / (10 | 60) entries, count a multiple of it); as_tasks
 *                   1: the models packed into LMTask / SFocalLMTask records and handed over as lm_tasks instead of models (no
 *                   refinement runs); thr2.  Outputs: out_counts, out_sums capacity each
 *   mask            models: one model; thr2.  Outputs: out_mask (device), out_host_mask (pinned mirror), capacity bytes each
 * Prefill before the launch: 0xff bytes in the counters (out_num_models, out_host_num_models, out_counts), 0x5a bytes - a finite
 * double - everywhere else.
 * PL_ERR_INVALID: a null argument, mixed or unsupported problem kinds, group 0 with more than one member, count 0 (unless idle) or
 * above 2^20, capacity below count, samples together with positions or neither, a sample index >= n, positions on a problem smaller
 * than a sample, a gate on a slot count that is no multiple of the models per iteration. */
typedef struct pl_focal_stage_member {
    pl_problem *problem;
    int32_t idle, as_tasks;
    uint32_t count, capacity;
    const uint32_t *samples, *positions;
    uint64_t seed, pos_base;
    double max_focal, thr2;
    const double *models;
    const uint32_t *num_models;
    double *out_models, *out_host_models;
    uint32_t *out_num_models, *out_host_num_models;
    uint32_t *out_counts;
    double *out_sums;
    uint8_t *out_mask, *out_host_mask;
} pl_focal_stage_member;
int pl_debug_focal_stage(int stage, int group, int workgroup_per_model, pl_focal_stage_member *members, size_t num_members);
/* Diagnostic entry (no counterpart in the reference): `n` models - pl_camera_pose[n] for kinds 0/1, double[n][9]
 * column-major for kinds 2/3 - through the STREAMING scorer of the batched main loop, i.e. through the conservative
 * pre-filters (fp16/MFMA or fp32) in front of the exact fp64 evaluation, instead of the sequential scorer behind
 * pl_score_model.  counts / scores: n entries each (scores summed in tree order: equal to pl_score_model's to rounding,
 * counts exactly).  path_used: 2 = matrix-core filter (k_score_mfma: absolute pose; k_score_mfma2: Sampson scores on
 * coordinates bounded by 8), 1 = fp32 filter (k_score_queue), 0 = no filter
 * (threshold / coordinates outside the filters' range, or POSELIB_AMD_NO_PREFILTER).  tests/ plants adversarial
 * models and correspondences here to check that a filter never drops an inlier. */
int pl_debug_score_stream(pl_problem *p, const void *models, size_t n, double max_error, uint32_t *counts,
                          double *scores, int32_t *path_used);
/* Diagnostic: how the streaming scorers cut n_points correspondences of a problem of `kind` (0 .. 5) - *chunks chunks of
 * 64 * *points_per_lane correspondences (on the matrix-core forms: 2 * points_per_lane groups of 32) - on the fp32-queue form
 * (matrix_core 0) or the matrix-core form (1), in the single-problem launch (group_form 0) or as a member of a lock-step group (1).
 * Like pl_debug_group_slices it assumes coordinates and threshold in the pre-filters' range, so the kind, the size and
 * POSELIB_AMD_NO_MFMA decide whether a matrix-core form exists: where none does, matrix_core 1 returns PL_ERR_UNSUPPORTED.  Kinds 4
 * (tangent) and 5 (1D-radial) have neither a matrix-core nor a group form: PL_ERR_INVALID, as for n_points 0 or an unknown kind.
 * Host arithmetic only: no device is touched.  tests/ derives its point counts from this entry. */
int pl_debug_score_shape(int kind, uint32_t n_points, int matrix_core, int group_form, uint32_t *chunks,
                         uint32_t *points_per_lane);
/* Diagnostic: pl_debug_score_stream with the scorer's grid in the caller's hand, and the group form of the same kernels.
 * A member is one resident problem with a model list of its own (models / n / max_error / counts / scores as in
 * pl_debug_score_stream) and `slices`, the hypothesis slices - workgroups of 8 wavefronts - per chunk of correspondences:
 * 0 = the rule production uses (route 0: pl_debug_score_stream's; route 2: the group's rule for the chunk total of the launch),
 * 1 .. the launch's limit = a grid of exactly that many.  Out: path_used (as pl_debug_score_stream), slices_used, chunks.
 *   route 0  the single-problem launch; one member of any kind.  pl_debug_score_stream is this route with slices 0.
 *   route 2  the group form, kinds 0 - 3: a device-resident argument table whose slot 0 is INACTIVE - with buffers of its own,
 *            filled with a pattern; *idle_changed receives the number of 32-bit words the launches changed in them, which must
 *            be 0 - followed by the 1 .. 4 members, all of one kind.  Every member has buffers of its own; its list is prepared
 *            by the helpers route 0 uses (hypothesis-ordered copies, live list, fp16 operands) on the group's chunk shape, its
 *            table entry is wired as a batch step wires it, and the launches are the ones a group's batch step runs: the group
 *            scorer dispatch - matrix-core and fp32-queue members in one call, each kernel launched if a member needs it - and
 *            the group's finalize.  Members may differ in size, threshold, list length and scorer path.
 * Before the launch every (chunk, hypothesis) partial is set to all-ones: a partial no wavefront writes shows as a wrong count.
 * PL_ERR_INVALID: another route, slices beyond the limit, route 0 with more or fewer than one member, route 2 with no or more
 * than four members, members of different kinds, a tangent or 1D-radial member, an empty list or an empty problem. */
typedef struct pl_debug_score_member {
    pl_problem *problem;
    const void *models;
    size_t n;
    double max_error;
    uint32_t *counts; /* n entries, may be NULL */
    double *scores;   /* n entries, may be NULL */
    uint32_t slices;
    uint32_t slices_used; /* out */
    uint32_t chunks;      /* out */
    int32_t path_used;    /* out */
} pl_debug_score_member;
int pl_debug_score_stream_ex(int route, pl_debug_score_member *members, size_t num_members, uint32_t *idle_changed);
/* Diagnostic: the PRUNED form of the matrix-core absolute-pose scorer on a caller-given model list, whatever
 * the gate of the batch steps says of its length: the first `lead` live hypotheses against every chunk of correspondences; their
 * best count and score, with the incumbent's (init_max, init_min), place the split chunk c*; every hypothesis against the chunks in
 * front of c* through the matrix-core filter alone (survivor counts, an upper bound of the inlier counts); the positions those
 * counts cannot exclude - the pre-selection - against every chunk, exactly; finalize and the candidate scan of a batch step.  Behind
 * these launches the entry labels the pre-selected positions with the exact rule on their exact partials in front of c*: that label
 * is `kept`.  Routes and the inactive slot as in pl_debug_score_stream_ex (route 0: one member, the single launches;
 * route 2: 1 .. 4 members behind an inactive slot 0, the group launches).
 *   counts / scores  per hypothesis, as pl_debug_score_stream for a pre-selected one (every kept one is); a position dropped on its
 *                    survivor count reports no inliers: count 0, score n thr^2 - a count not above, a score not below the full ones
 *   kept             per hypothesis, 1 or 0: the exact rule (NaN models, never scored, report 1; cstar == chunks: all 1)
 *   cand             hypothesis indices of the candidates the scan lists, in the order it listed them (num_cand of them, at most
 *                    cand_cap are written)
 * PL_ERR_UNSUPPORTED: a member whose problem is not scored on the matrix cores.  PL_ERR_INVALID: as pl_debug_score_stream_ex, or a
 * member of another kind than absolute pose. */
typedef struct pl_debug_prune_member {
    pl_problem *problem;
    const void *models; /* pl_camera_pose[n] */
    size_t n;
    double max_error;
    double init_min;   /* the incumbent's score ... */
    uint32_t init_max; /* ... and inlier count: what a candidate has to beat */
    uint32_t cand_cap;
    uint32_t *counts; /* n entries, may be NULL */
    double *scores;   /* n entries, may be NULL */
    uint8_t *kept;    /* n entries, may be NULL */
    uint32_t *cand;   /* cand_cap entries */
    /* out */
    uint32_t num_cand;
    uint32_t cstar, chunks, chunk_points; /* the split chunk, the chunks of the launch and the correspondences of one */
    uint32_t lead;                        /* live positions of the lead */
    uint32_t lead_max;
    uint32_t num_live, num_selected;      /* hypotheses without a NaN entry; live hypotheses that are kept (0 when cstar == chunks) */
    uint32_t slices, num_preselected;     /* workgroups of 8 wavefronts per chunk of the count launch (the plain launch's; the lead
                                             runs on min(slices, 2), the exact launch on ceil(slices / 4)); live positions the exact
                                             launch scored: the lead and what the survivor counts could not exclude (this
                                             word was `pad`, always written 0: same offset and size, PL_ABI_VERSION stays) */
    double lead_min;
} pl_debug_prune_member;
int pl_debug_score_pruned(int route, pl_debug_prune_member *members, size_t num_members, uint32_t *idle_changed);
/* Diagnostic: the count launch of the pruned form alone - the matrix-core filter without the exact pass - over the whole list and
 * every chunk.  Members and routes as pl_debug_score_pruned: problem, models, n, max_error are read; chunks, chunk_points, num_live
 * and slices are written; no lead, selection or finalize runs, so every other field and array of a member is neither read nor
 * written.  survivors[i]: member i's [chunks][n] survivor counts in hypothesis order, chunks as pl_debug_score_shape
 * gives them for the route; a NaN model reports 0.  guard_changed: words of the count columns behind the live list's end that the
 * launch changed - which must be 0. */
int pl_debug_score_survivors(int route, pl_debug_prune_member *members, size_t num_members, uint32_t *const *survivors,
                             uint32_t *idle_changed, uint32_t *guard_changed);
/* Diagnostic: the pruned form as a batch step of a group launches it - pl_debug_score_pruned's sequence with the BOUND TIER between
 * pre-selection and exact scores, the lead left out of the exact launch, and no labels.  Members and routes as pl_debug_score_pruned.
 * Per member i and hypothesis k:
 *   bound_counts[i][k], bound_scores[i][k]   the tier's upper bound of the inlier count and lower bound of the score, for a
 *                    pre-selected position behind the lead - those of the last of the tier's three stages that saw it (the survivor
 *                    count over all n correspondences - bound_counts = that count c, bound_scores = (n - c) thr^2 rounded down -,
 *                    then the fp32 filter's verdict for what that leaves, then residual bounds for what the verdict leaves
 *                    undecided); 0xffffffff / NaN for every other hypothesis, and for all when the tier
 *                    does not run (cstar == chunks)
 *   tiers[i][k]      0: exact scores (the lead, and what both tiers kept); 1: dropped on its survivor count; 2: dropped on its
 *                    bounds; 3: NaN model, never scored
 *   counts / scores / cand as pl_debug_score_pruned - a dropped position reports count 0, score n thr^2; kept: tiers == 0 or 3;
 *                    num_selected: live hypotheses with exact scores; num_preselected: the entries the exact launch scored (without
 *                    the lead when the tier ran).
 * guard_changed: words of the count columns behind the live list's end that the launches changed - which must be 0. */
int pl_debug_score_bounded(int route, pl_debug_prune_member *members, size_t num_members, uint32_t *const *bound_counts,
                           double *const *bound_scores, uint8_t *const *tiers, uint32_t *idle_changed, uint32_t *guard_changed);
/* Diagnostic: pl_debug_score_bounded, and the count columns as its launches left them.  columns[i]: member i's [chunks][n] words in
 * hypothesis order (a NaN model reports 0): exact inlier counts for a hypothesis with exact scores (tiers 0); for one dropped on its
 * bounds (tiers 2) the matrix-core filter's survivor count of every chunk - the count launch's in front of cstar, from cstar on those
 * of the launch that counts the pre-selection behind the lead for stage S of the bound tier; for one dropped on its survivor count
 * (tiers 1) survivor counts in front of cstar and, from cstar on, whatever the column held before the step.  A new entry point next
 * to an unchanged one: PL_ABI_VERSION stays 5. */
int pl_debug_score_bounded_columns(int route, pl_debug_prune_member *members, size_t num_members, uint32_t *const *bound_counts,
                                   double *const *bound_scores, uint8_t *const *tiers, uint32_t *const *columns, uint32_t *idle_changed,
                                   uint32_t *guard_changed);
/* Diagnostic: 1 if a batch step of `iterations` iterations of a problem of `kind` with n_points correspondences, as a member of a
 * lock-step group (pl_ransac_batch, pl_estimate_batch), scores in the pruned form, 0 if not; pl_ransac_run's own steps never do (coordinates and threshold in the pre-filter's range assumed, as pl_debug_group_slices).  Host arithmetic only. */
int pl_debug_score_prune_gate(int kind, uint32_t n_points, uint32_t iterations);
/* Diagnostic: the kernel that refines ONE camera-less job of max_iterations LM iterations on a problem of `kind` with n_points
 * correspondences (pl_refine_model, a local optimisation of pl_ransac_run) under the process's current LM mode (pl_set_lm_mode) and
 * latency setting (POSELIB_AMD_LATENCY_MODE, read once): 0 k_lm - one workgroup; sums in the reference's order up to 256
 * correspondences, tree sums beyond -, 1 k_lm_ordered - every sum in the reference's order -, 2 k_lm2 - *slices workgroups per
 * task, one launch per iteration; *slices is 0 for the other two.  The function the driver itself asks.  PL_ERR_INVALID: unknown
 * kind, n_points 0, slices NULL.  Host arithmetic only: no device is touched. */
int pl_debug_lm_route(int kind, uint32_t n_points, uint64_t max_iterations, uint32_t *slices);
/* Diagnostic: the shape of the device sampler (k_sample_delta / k_sample_orbit) for a batch of B iterations of samples of K out of N
 * correspondences.  window: the draw positions a batch step evaluates, as the driver sizes them (the argument `window` 0), or the
 * caller's.  build: the build of the orbit kernel the launcher picks for (window, N, K) - 1 small, 2 large; a group's launch picks
 * one build for (largest window, smallest N) of its members.  Per build: the flagged positions it holds, the most of them pointer
 * doubling follows (more, up to `flags`: the one-lane walk) and the segments of its table.  tile: positions per tile of the ordered
 * append.  PL_ERR_INVALID: K outside {3, 4, 5, 7}, N < K, B == 0.  Host arithmetic only: no device is touched.  tests/ takes every
 * one of these numbers from here. */
typedef struct pl_debug_sampler_shape_info {
    uint64_t window;
    uint32_t build, tile;
    uint32_t small_flags, small_doubling, small_segments;
    uint32_t large_flags, large_doubling, large_segments;
} pl_debug_sampler_shape_info;
int pl_debug_sampler_shape(int K, uint64_t N, uint32_t B, uint64_t window, pl_debug_sampler_shape_info *out);
/* Diagnostic: the device sampler on its own.  A member is one draw stream (seed, pos_base), N correspondences, B iterations and a
 * window of M positions (0: the driver's, pl_debug_sampler_shape's `window`; M_used returns it - size delta and flagbits by it).
 *   drawn    (planted NULL) k_sample_delta<K> evaluates the window and clears the control block, k_sample_orbit walks it: the two
 *            kernels of a batch step, through their launcher.
 *   planted  M bytes: the delta table itself - draws an iteration starting at each position consumes, K for an ordinary one.  The
 *            entry uploads it with the bitmap of delta != K (no bit at or behind M), clears the control block with a memset, as a
 *            step whose positions come from the host does, and launches the orbit kernel alone: tables no draw stream produces.
 *   route 0  one single-problem launch per member, one after the other.
 *   route 2  the group form: a device-resident table whose slot 0 is INACTIVE, with pattern-filled buffers of its own
 *            (*idle_changed: the 32-bit words the launches changed in them, which must be 0), then the 1 .. 4 members, wired as a
 *            batch step wires them, in ONE launch; all drawn or all planted.
 *   build    0: as the launcher picks it (route 2: for the largest window and the smallest N), 1: small, 2: large.
 * Every member has buffers of its own, filled with the byte 0xa5 first; positions are set to all-ones.  Out, per member: positions
 * (B words, relative to pos_base; unspecified where orbit_error is set), delta (M bytes), flagbits (M / 64 + 2 words: the bitmap's
 * ceil(M / 64) words and what lies behind them, which must still be the pattern), pos_after, orbit_error, build_used, delta_guard (1:
 * the 64 bytes behind delta[M] kept the pattern), ctl_clear (1: apart from pos_after and orbit_error every word of the control block
 * and of the tables behind it is zero, and the word behind them kept the pattern).
 * PL_ERR_INVALID: another route or build, no or more than four members, K outside {3, 4, 5, 7}, N < K or N >= 2^32, B == 0 or
 * B > 2^20, M > 2^31 - 1, pos_base + M >= 2^32 - 1 (the driver's own limits), a missing positions pointer, drawn and planted members
 * in one group. */
typedef struct pl_debug_sampler_member {
    uint64_t seed, pos_base, N;
    uint32_t B, M;
    const uint8_t *planted; /* NULL: drawn */
    uint32_t *positions;    /* out: B words */
    uint8_t *delta;         /* out: M bytes, may be NULL */
    uint64_t *flagbits;     /* out: M / 64 + 2 words, may be NULL */
    /* out */
    uint64_t pos_after;
    uint32_t orbit_error, M_used, build_used;
    int32_t delta_guard, ctl_clear, pad;
} pl_debug_sampler_member;
int pl_debug_sample_positions(int route, int K, int build, pl_debug_sampler_member *members, size_t num_members, uint32_t *idle_changed);
/* Diagnostic entry: the scalar math of the device kernels, element-wise on `n` doubles (n <= 2^28) - fn 0: the cube of
 * the LM's Nielsen update (optim/lm_impl.h:124 std::pow(., 3)), 1: sqrt, 2: reciprocal, 3 .. 6: cbrt / cos / sin / acos
 * of pl_libm.h, 7 / 8: sine / cosine of pl_sincos (the quaternion exponential of the LM steps), 9: pf_half_rn((float)x),
 * 10: pf_half_to_float((uint16_t)x), 11: pf_half_up((float)x) - the fp16 operand conversions of the matrix-core
 * pre-filters, fp16 bit patterns passed and returned as their integer value.  Any other fn: PL_ERR_INVALID.
 * cos and sincos follow glibc for |x| < 105414350, sin for |x| < 2.426265 (pl_libm.h); beyond, they return the device
 * library's values.  tests/ compares every code with the host's libm / IEEE arithmetic bit for bit. */
int pl_debug_device_math(int fn, const double *x, size_t n, double *out);
/* ... and the two functions the fisheye cameras need, element-wise on n <= 2^28 pairs - fn 0: out[i] = pl_atan2(x[i], y[i])
 * (x is atan2's FIRST argument, the cameras' rho), fn 1: out[i] = pl_tan(x[i]) (y is not read and may be NULL).  Any other fn:
 * PL_ERR_INVALID.  pl_atan2 follows glibc for every finite second argument and every finite non-zero first one, pl_tan for
 * |x| <= 25 (pl_libm.h); beyond, they return the device library's values (finite input: finite or +-inf as tan goes). */
int pl_debug_device_math2(int fn, const double *x, const double *y, size_t n, double *out);
/* Non-linear refinement of one model on the resident correspondences (robust/bundle.h:41-170:
 * bundle_adjust / refine_relpose / refine_fundamental / refine_homography).  camera: absolute pose only
 * (NULL pointer = identity camera, i.e. normalised image points; otherwise any supported model, the points being its
 * pixels).  mask: optional N bytes, refine on the
 * flagged correspondences only. */
int pl_refine_model(pl_problem *p, const pl_bundle_options *opt, const pl_camera *camera, const uint8_t *mask,
                    void *model, uint32_t *lm_iterations);

/* bundle_adjust(x, X, Image *image, BundleOptions) - the Image overload of robust/bundle.h:47-49 / bundle.cc:94-113 - on
 * an absolute-pose problem whose 2-D points are PIXELS: pose and, per opt->refine_focal_length / refine_principal_point /
 * refine_extra_params, the camera's intrinsics are refined together (robust/optim/absolute.h:49-171); both in / out.
 * The flags select parameters in the reference's order (Camera::get_param_refinement_idx): focal, principal point, extra -
 * SIMPLE_RADIAL {0}, {1, 2}, {3}; RADIAL {0}, {1, 2}, {3, 4}; OPENCV {0, 1}, {2, 3}, {4 .. 7}; OPENCV_FISHEYE {0, 1}, {2, 3},
 * {4 .. 7}; SIMPLE_RADIAL_FISHEYE {0}, {1, 2}, {3}; RADIAL_FISHEYE {0}, {1, 2}, {3, 4}. */
int pl_bundle_adjust_camera(pl_problem *p, const pl_bundle_options *opt, pl_camera *camera, const uint8_t *mask,
                            pl_camera_pose *pose, uint32_t *lm_iterations);

/* ---- minimal solvers (solvers/ headers); unit bearing vectors in, solutions out; return = #solutions or <0 ---- */
int pl_p3p(const double *x /* 3x3 */, const double *X /* 3x3 */, pl_camera_pose *out /* 4 */);
/* p5lp_radial (solvers/p5lp_radial.h:49, the 2-D point form; a radial line l is the point (l_y, -l_x)): poses with t[2] = 0 */
int pl_p5lp_radial(const double *x /* 5x2 */, const double *X /* 5x3 */, pl_camera_pose *out /* 4 */, int *count /* may be null */);
int pl_relpose_5pt(const double *x1 /* 5x3 */, const double *x2 /* 5x3 */, pl_camera_pose *out /* 40 */);
int pl_essential_matrix_5pt(const double *x1, const double *x2, double *E /* 10 x 9 column-major */);
int pl_relpose_7pt(const double *x1 /* 7x3 */, const double *x2 /* 7x3 */, double *F /* 3 x 9 column-major */);
int pl_homography_4pt(const double *x1 /* 4x3 */, const double *x2 /* 4x3 */, double *H /* 9 column-major */);
/* the solvers of the two focal-length estimators (interfaces of solvers/p35pf.h:39-54 and solvers/relpose_6pt_focal.h:12-13; the
 * algorithms restate the reference's action-matrix templates since round 6 and return its roots in its order).  pl_p35pf: x = four image points relative to the principal point
 * (4 x 2; of the fourth only x is used), X = 4 x 3; out / focals: room for 10.  pl_relpose_6pt_shared_focal: six pairs of unit
 * bearings (6 x 3 each); out / focals: room for 60, in the reference's order.  Return = #solutions or < 0. */
int pl_p35pf(const double *x, const double *X, pl_camera_pose *out, double *focals);
int pl_relpose_6pt_shared_focal(const double *x1, const double *x2, pl_camera_pose *out, double *focals);
/* batched: kind 0 = P3.5Pf (in: count x [x 4 x 2 | X 4 x 3]; 10 slots), kind 1 = 6-point shared focal (in: count x [x1 6 x 3 |
 * x2 6 x 3]; 60 slots); out_models: count x slots x 8 doubles (q[4] t[3] focal), out_counts: count. */
int pl_solve_focal_batch(int kind, const double *in, size_t count, double *out_models, uint32_t *out_counts);
/* batched form: `count` independent minimal problems, one GPU lane each.
 * in: count x (2*K*3) doubles ([first set K x 3][second set K x 3]); out_models: count x max_models x 24 doubles
 * (model records of 24 doubles: q[4] t[3] M[9 row-major] + 8 doubles of internal fp32 shadow, see
 * poselib_amd/csrc/pl_math.h); out_counts: count. */
/* kind 5: p5lp_radial - first set = the 2-D points as K x 3 (third component not read), K = 5, max_models 4 */
int pl_solve_batch(int kind, const double *in, size_t count, double *out_models, uint32_t *out_counts);

#ifdef __cplusplus
}
#endif
#endif /* POSELIB_AMD_H_ */
