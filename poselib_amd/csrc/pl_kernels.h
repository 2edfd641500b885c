// poselib_amd — launch interface between the host driver (driver.cc) and the HIP kernels
// (kernels.hip).  Plain structs and pointers only.
#pragma once
#include "pl_prefilter.h"
#include "pl_refine.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pl {

// Correspondences of one problem, structure-of-arrays in HBM, fp64.
//   absolute pose : a[0..4] = x, y (normalised image plane), X, Y, Z
//   1D-radial absolute pose (EST_RAD1D): a[0..4] = x, y (centred pixels times the front-end's scale), X, Y, Z
//   two-view      : a[0..3] = x1, y1, x2, y2
//   tangent Sampson (EST_RELT): a[0] = the block of 18 arrays d1[3] d2[3] M1[6] M2[6], component c at a[0] + c * n
struct PointSet {
    const double *a[5];
    uint32_t n;
    float xy_absmax; // absolute pose: max(|x|, |y|) over the 2-D points; two-view: max over all four coordinates, +inf
                     // when unknown (bounds used by the scoring pre-filters)
};

constexpr int kScoreThreads = 256; // 4 wavefronts per workgroup
constexpr int kStreamWaves = 8;    // wavefronts per workgroup of the streaming scorers (kQueueThreads, kMfmaThreads in kernels.hip)
constexpr int kLMSeqPoints = 256; // up to this many correspondences k_lm sums in the reference's order (one thread per correspondence)
#ifndef PL_LM_THREADS
#define PL_LM_THREADS 512
#endif
constexpr int kLMThreads = PL_LM_THREADS; // k_lm: wavefront 0 adds the term rows in order, the others produce them (kernels.hip)

PL_HD constexpr int sample_size(int est) { return est == EST_ABS ? 3 : (est == EST_REL || est == EST_RELT || est == EST_RAD1D) ? 5 : est == EST_FUND ? 7 : 4; }
PL_HD constexpr int max_models(int est) { return (est == EST_ABS || est == EST_RAD1D) ? 4 : (est == EST_REL || est == EST_RELT) ? 40 : est == EST_FUND ? 3 : 1; }
PL_HD constexpr int point_doubles(int est) { return (est == EST_ABS || est == EST_RAD1D) ? 5 : est == EST_RELT ? 18 : 4; }

struct BatchCtl;
struct GenerateArgs {
    PointSet pts;
    uint64_t seed;
    uint64_t pos_base;         // draws consumed before the batch
    const uint32_t *positions; // draws consumed before each iteration, relative to pos_base
    const uint32_t *samples;   // optional explicit minimal samples [num_iters][K] (PROSAC: drawn on the host,
                               // the subset schedule is a serial recurrence); nullptr => draw from `positions`
    uint32_t num_iters;
    uint32_t slots_per_iter;   // record slots reserved per iteration (<= max_models(est)); more solutions than
                               // slots => ctl->gen_overflow is set and the host repeats the batch with more room
    struct BatchCtl *ctl;
    double *models;            // [num_iters * slots_per_iter] records of kModelStride doubles
    uint32_t *num_models;      // [num_iters]
    int32_t real_focal_check;  // fundamental only
    uint32_t *blk_tot = nullptr; // optional, zeroed: models per block of 1024 iterations, accumulated by the generator
    uint32_t *blk_nan = nullptr; // optional, zeroed: NaN models per block of 1024 iterations (statistics)
    uint32_t *nan_bits = nullptr; // optional [num_iters], absolute pose only (<= 4 slots per iteration - the one kind that builds a
                               // live list): bit m = model m of the iteration carries the NaN flag.  Every iteration writes its
                               // entry, so the array needs no clearing; k_compact2 reads it instead of the records' flag words
    void *stage = nullptr;     // relative pose: workspace of generate_stage_bytes(); nullptr = single-kernel generator
};

// ---- k_score_mfma with pruning: hypotheses that provably cannot become candidates of k_records are not
// scored exactly at all.  lead -> (lead_max, lead_min, c*) -> survivor counts of the matrix-core filter (the list behind the lead,
// chunks [0, c*)) -> pre-selection of the positions the counts cannot exclude -> fp32 bounds of count and score of the pre-selected
// positions behind the lead (every chunk), which drop what cannot beat the lead -> exact scores (what is left, every chunk).
constexpr uint32_t kPruneLead = 2048;   // live positions scored against every chunk first (a prefix of the hypothesis order)
constexpr uint32_t kPruneMargin = 32;   // correspondences added to the bound that places c*
constexpr double kPruneScoreMargin = 1e-6; // relative margin of the score test (k_records compares with 1e-9)
struct PruneState { // device memory, one per problem and step
    uint32_t lead_max; // best count of the incumbent and the lead
    uint32_t cstar;    // the split chunk, 1 .. chunks; chunks: nothing is pruned
    uint32_t sel_len;  // length of the selection list
    uint32_t pad;
    double lead_min;   // best score of the incumbent and the lead
};
struct PruneArgs {
    PruneState *st = nullptr;  // nullptr: the step scores every live hypothesis against every chunk
    uint32_t *blk_kept = nullptr; // [ceil(hyp_capacity / 1024)] kept positions per tile of 1024 live positions
    uint32_t *sel = nullptr;   // [hyp_capacity] kept live positions, ascending
    uint8_t *kept = nullptr;   // [hyp_capacity] per live position: kDropped - no exact partials, kKept - pre-selected: exact
                               // partials of every chunk; kPrunedExact: pl_debug_score_pruned's label, see k_prune_label
    uint32_t chunks = 0, chunk_points = 0; // the launch's chunks of correspondences and the correspondences of one
    uint32_t init_max = 0, lead = 0;   // what a candidate has to beat (RecordsArgs.init_max / init_min); lead length
    double init_min = 0.0;
    // The bound tier (kScoreCountSel's survivor counts, k_score_bound: three stages in one launch, k_prune_bound) between pre-selection and exact scores; 0: the two-tier sequence, the lead
    // stays in the selection (pl_debug_score_pruned, pl_debug_score_survivors)
    uint32_t bound = 0, pad = 0;
    uint32_t *bnd_count = nullptr; // optional (pl_debug_score_bounded) [hyp_capacity]: per pre-selected position behind the lead
    double *bnd_score = nullptr;   // the tier's upper bound of the count and lower bound of the score
};
constexpr uint8_t kDropped = 0, kKept = 1, kPrunedExact = 2;

struct ScoreArgs {
    PointSet pts;
    const double *models;
    const uint32_t *slots;     // hypothesis k -> model record index (nullptr: identity); k_score_mfma: the LIVE list
                               // (record index of every hypothesis without the NaN flag, in hypothesis order)
    const float *shadow;       // optional compact [num_hyp][16] fp32 model shadows in hypothesis order (pre-filter)
    const double *compact64;   // optional compact [num_hyp][16] fp64 model fields in hypothesis order (pre-filter)
    const void *shadow16;      // optional fp16 MFMA operand blocks of the hypotheses (absolute pose, k_score_mfma):
                               // 64 B per LIVE hypothesis, see shadow16_one in pipeline.hip
    const void *points16 = nullptr; // k_score_mfma: fp16 operand rows of the correspondences (kAbs16PointBytes each, one per
                               // correspondence of every chunk, see abs16_point_row in pipeline.hip)
    const uint32_t *num_hyp;   // device scalar; k_score_mfma: BatchCtl.num_live, the length of the live list
    uint32_t hyp_capacity;     // row pitch of the partial arrays
    double thr2;
    PrefilterArgs pf;          // conservative fp32 pre-filter (pl_prefilter.h); pf.enabled == 0: exact evaluation
    uint32_t *part_count;      // [chunks][hyp_capacity]
    double *part_score;        // [chunks][hyp_capacity]
    uint32_t *tickets;         // [chunks], zeroed before the launch: work counters of the waves that share a chunk
    PruneArgs prune;           // k_score_mfma only; prune.st == nullptr: everything is scored
};
constexpr uint32_t kMaxScoreChunks = 4096; // (2^31 correspondences / 64 P would be more; the driver rejects such sets)

constexpr uint32_t kNoRank = 0xffffffffu; // rank[] of a NaN hypothesis: it has no row in the live list
struct FinalizeArgs {
    const uint32_t *num_hyp;
    const uint32_t *rank = nullptr; // k_score_mfma: hypothesis k -> its position in the live list, the column of its partials
                                    // (kNoRank: NaN model, no inliers); nullptr: the partials are indexed by k
    uint32_t hyp_capacity, chunks, n_points;
    double thr2;
    const uint32_t *part_count;
    const double *part_score;
    uint32_t *count; // [hyp_capacity]
    double *score;   // [hyp_capacity]
    // pruned step (PruneArgs): a live position with kept[] == kDropped has no partials (its count column holds survivor counts
    // or an earlier step's values) and reports no inliers.  nullptr: every column holds all chunks
    const uint8_t *kept = nullptr;
};

struct LMTask {
    PointSet pts;                 // the correspondences the task refines on
    double params[kParamDoubles]; // in/out (see pl_refine.h for the per-problem layout)
    LMOptions opt;
    CameraParams cam;      // absolute pose only
    double point_scale;    // absolute pose: 2-D points are multiplied by this on load (final bundle)
    double prefilter_thr2; // relative pose LO: > 0 => keep only points passing Sampson+cheirality at this
                           // threshold; skip the refinement when <= 5 survive (relative_pose.cc:62-86)
    const uint8_t *mask;   // optional inlier mask (final polish on inliers); nullptr = all points
    uint8_t *scratch;      // n bytes, used by the prefilter
    const double *record_in; // k_lm: the seed's model record (kept when the refinement is skipped) ...
    double *record_out;      // ... and where the refined model's record goes (device memory); nullptr: no record
    int32_t cam_flags;       // k_lm_cam: CamRefineFlags (pl_refine_cam.h) - the intrinsics refined with the pose; `cam` is in/out
    int32_t pad0;
    // A task that is enqueued BEHIND the kernels that decide whether and from where it runs (pl_estimate_batch: the front-end's final
    // bundle behind the final refinement, its choice and the inlier mask - one synchronisation instead of two):
    const double *start_record;  // optional: the model record (device memory) whose parameters replace `params` as the starting point
    const uint32_t *gate_count;  // optional: the task runs only if *gate_count > gate_min (robust.cc:103 "num_inliers > 3" etc.); otherwise
    uint32_t gate_min;           // skipped = 2 and nothing else is written
    uint32_t pad1;
    // outputs
    uint32_t iterations, skipped;
    double cost, initial_cost;
};

// Device-resident control block of one batch (zeroed before the batch, read back after it).
struct BatchCtl {
    uint32_t num_hyp;     // hypotheses of the batch (k_compact2)
    uint32_t num_records; // improving hypotheses found by k_records (may exceed the list capacity)
    uint32_t orbit_error; // sampler position window too small / too many redraw segments
    uint32_t gen_overflow; // an iteration produced more models than slots_per_iter
    uint64_t pos_after;   // draws consumed after the batch's last iteration
    uint32_t nan_hyp;     // hypotheses of the batch with a NaN entry (counted by the generators, summed by k_compact2;
                          // the scorers skip them: no inliers)
    uint32_t num_live;    // hypotheses without the NaN flag = length of the live list the matrix-core absolute-pose scorer
                          // runs over (k_compact2; 0 where no live list is built)
};
struct RecordMeta {
    uint32_t k, slot, count, pad;
    double score;
};

// k_score_seq: scores in the reference's (sequential) summation order for the models decisions are taken on.
struct SeqScoreArgs {
    PointSet pts;
    const double *models;   // records of kModelStride doubles
    RecordMeta *cand;       // candidate list: model of candidate r = models + cand[r].slot; count / score are rewritten.
                            // nullptr: model r = models + r, results go to count[] / score[]
    const uint32_t *num;    // number of candidates / models (device memory)
    uint32_t cap;           // upper bound of *num
    double thr2;
    uint32_t *count;        // plain mode: [cap]
    double *score;          // plain mode: [cap]
    uint32_t *host_count;   // plain mode: optional pinned mirrors
    double *host_score;
    RecordMeta *host_cand;  // candidate mode: pinned mirror of the first host_cap candidates
    uint32_t host_cap;
    const BatchCtl *ctl_src = nullptr; // optional: the batch's control block, final when this kernel starts, is copied
    BatchCtl *ctl_host = nullptr;      // to pinned host memory by the kernel itself (no copy dispatch)
};
hipError_t launch_score_seq(int est, const SeqScoreArgs &a, hipStream_t stream);

// All launchers enqueue on `stream` and return the HIP status of the launch.
hipError_t launch_generate(int est, const GenerateArgs &a, hipStream_t stream);
size_t generate_stage_bytes(int est, uint32_t num_iters); // workspace of the staged 5-point generator (0: none)
// the staged 5-point generator (gen_rel.hip): a.stage = workspace of rel_stage_bytes(a.num_iters)
size_t rel_stage_bytes(uint32_t num_iters);
// tangent: the correspondences are an EST_RELT block and its bearings are the solver's input (k_rel_front_tangent)
hipError_t launch_generate_rel(const GenerateArgs &a, hipStream_t stream, bool tangent = false);
struct GroupArgs;
hipError_t launch_group_generate_rel(const GroupArgs *args, uint32_t max_B, uint32_t G, hipStream_t stream);
// the generator launch of a group's batch step on its own (kinds 0 - 3; launch_group_batch and the diagnostic entry pl_debug_generate)
hipError_t launch_group_generate(int est, const GroupArgs *args, uint32_t max_B, uint32_t G, hipStream_t stream);
// Front-end pre-processing on the device (robust.cc:40-46, 286-292; utils.cc:584-644 per-point part): AoS user
// buffers -> the problem's SoA block, with per-point un-projection (modes 0, 1) or the affine normalisation whose
// centroid / scale the host has summed sequentially (mode 2; the two reductions of normalize_points are order
// dependent and stay on the host to remain bit-identical).  absmax_bits: max(|x|, |y|) of the first point set as the
// bit pattern of a non-negative double (NaN propagates), zeroed by the caller.
struct PrepareArgs {
    int32_t mode;          // 0: a -> unproject(cam1), b = N x 3 copied; 1: a -> unproject(cam1), b -> unproject(cam2);
                           // 2: a -> (a - c1) / scale, b -> (b - c2) / scale   (subtract only if `centred`)
                           // 3: tangent Sampson - a, b multiplied by `scale`, then bearing and Jacobian of the un-projection
                           //    through cam1 / cam2 (already rescaled): the 18 arrays of an EST_RELT problem
    int32_t centred;
    CameraParams cam1, cam2;
    double c1x, c1y, c2x, c2y, scale;
};
hipError_t launch_prepare(const double *a_raw, const double *b_raw, uint32_t n, const PrepareArgs &args, double *soa,
                          unsigned long long *absmax_bits, hipStream_t stream);
// pixels of a distorting camera -> pixels of the distortion-free camera with the same focal lengths / principal point
// diagnostic: fn 0 cube of the LM's Nielsen update, 1 sqrt, 2 reciprocal, 3 cbrt, 4 cos, 5 sin, 6 acos, 7 / 8 sin / cos of
// sincos, 9 fp16 round-to-nearest bits, 10 fp16 bits -> float, 11 fp16 round-up bits - as the kernels evaluate them
constexpr int kDeviceMathFns = 12;
hipError_t launch_device_math(int fn, const double *x, uint32_t n, double *out, hipStream_t stream);
// diagnostic, two arguments: fn 0 pl_atan2(x, y), 1 pl_tan(x) (y not read)
constexpr int kDeviceMath2Fns = 2;
hipError_t launch_device_math2(int fn, const double *x, const double *y, uint32_t n, double *out, hipStream_t stream);
hipError_t launch_undistort(const double *in, uint32_t n, const CameraParams &cam, double fx, double fy, double cx,
                            double cy, double *out, hipStream_t stream);
// ---- correspondences in the caller's device memory (ingest.hip): rows of `cols` contiguous fp32 / fp64 elements, row_stride
// elements apart (pl_device_points once the driver has checked it)
struct IngestSrc {
    const void *data;
    int64_t row_stride;
    int32_t f32; // elements are float (widened exactly), otherwise double
    int32_t cols;
};
// -> the contiguous fp64 AoS blocks k_prepare / k_prepare_tangent take (n x a.cols, n x b.cols)
hipError_t launch_ingest(const IngestSrc &a, const IngestSrc &b, uint32_t n, double *out_a, double *out_b, hipStream_t stream);
// -> the SoA block of a resident problem (a.cols + b.cols arrays of n) and, like make_problem, max |a| - with max |b| when
// b_in_max - as an atomic max of bit patterns on *absmax_bits (zeroed by the caller; a NaN propagates; null: no maximum).
// scale_a: a's columns are multiplied by it on their way in, the maximum is the products' (the 1D-radial front-end)
hipError_t launch_ingest_soa(const IngestSrc &a, const IngestSrc &b, uint32_t n, int b_in_max, double *soa,
                             unsigned long long *absmax_bits, hipStream_t stream, double scale_a = 1.0);
// What the front-ends compute over the raw points on the host, from the fp64 AoS blocks (N x 2 each) on the device:
//   norm     1: the two order-dependent reductions of the homography / fundamental normalisation (utils.cc:584-644) in index order;
//            2: the second of them about the GIVEN centres c1 = (cx1, cy1), c2 = (cx2, cy2) - no centroid pass (shared focal,
//            normalization_about); 3: one point set (b_raw is not read): scale = n / sum_k sqrt(0.0 + x_k^2 + y_k^2) in index order
//            and absmax = max |coordinate * scale|, NaN propagating (the 1D-radial front-end and make_problem's bound); no `bound`
//   bound    0 none; 1 max |(a - c1) / f1| (absolute pose, linear camera); 2 the same over both sets with their cameras (relative
//            pose, linear cameras); 3 max |(x - centroid) / scale| with the centroids and scale of `norm` (requires norm)
struct PointStatsArgs {
    int32_t norm, centred, bound, pad;
    double cx1, cy1, fx1, fy1, cx2, cy2, fx2, fy2; // bound 1 / 2
    double n_as_double, scale_divisor;             // norm: n and sqrt(2) * n as the host forms them
};
struct PointStatsRecord { // what the call reads back
    double c1x, c1y, c2x, c2y, scale, absmax, reserved[2];
};
hipError_t launch_point_stats(const double *a_raw, const double *b_raw, uint32_t n, const PointStatsArgs &args,
                              PointStatsRecord *out /* device-visible */, hipStream_t stream);
// The two for the members of a lock-step group (pl_estimate_batch_dev): one launch each, the member is blockIdx.z.  The tables are
// device-visible (pinned and mapped, or device memory); the pointers in them are read as global memory.
struct IngestGroupArgs {
    IngestSrc a, b;
    uint32_t n, pad;       // rows; 0: nothing to copy for this member (both sets are read where they lie)
    double *out_a, *out_b; // the member's slices of the group's raw block; null: that set is contiguous fp64 and read in place
};
// blocks beyond a member's n return; max_n: the largest n of the table
hipError_t launch_ingest_g(const IngestGroupArgs *tab, uint32_t G, uint32_t max_n, hipStream_t stream);
struct PointStatsGroupArgs {
    const double *a_raw, *b_raw; // fp64 AoS blocks (N x 2 each): the ingested slices or the caller's memory
    uint32_t n, pad;             // 0: the host has no pass over this member's points - no work, no record
    PointStatsArgs args;
    PointStatsRecord *out;       // device-visible
};
hipError_t launch_point_stats_g(const PointStatsGroupArgs *tab, uint32_t G, hipStream_t stream);
// The un-distortion stage (launch_undistort) from the caller's device rows into the caller's fp64 rows (ingest.hip): one member of
// pl_undistort_points_batch_dev, or the arguments of the single call
struct UndistortDevArgs {
    IngestSrc src;         // N x 2
    uint32_t n, pad;       // rows; 0: no work
    CameraParams cam;
    double fx, fy, cx, cy; // the distortion-free camera the output pixels belong to
    double *out;           // columns 0 and 1 of row i are written, nothing else
    int64_t out_stride;    // ELEMENTS between rows, >= 2
};
hipError_t launch_undistort_dev(const UndistortDevArgs &args, hipStream_t stream);
// member = blockIdx.z, device-visible table; max_n: the largest n of the table
hipError_t launch_undistort_dev_g(const UndistortDevArgs *tab, uint32_t G, uint32_t max_n, hipStream_t stream);
// ---- one confidence per row next to the correspondences (rank.hip; pl_device_scores once the driver has checked it).  The rule:
// row i is kept iff score[i] >= min_score (a NaN never is); kept rows go in descending score, equal scores (-0.0 == 0.0) in ascending
// row index.  fp32 scores widen exactly, so one 64-bit key serves both dtypes and the pair (key, row) is a total order: the
// permutation does not depend on how it is computed.
struct RankSrc {
    const void *data;
    int64_t stride; // ELEMENTS between consecutive scores
    int32_t f32, pad;
    double min_score;
};
struct RankArgs {
    RankSrc s;
    uint32_t n, pad;
    unsigned long long *keys[2]; // members beyond one tile: the two sides of the merge passes, n entries each; otherwise unused
    uint32_t *rows[2];
    uint32_t *order; // out: n slots, the first *kept are written
    uint32_t *kept;  // out, device-visible
};
// rows one workgroup sorts in LDS for a launch whose largest member has max_n rows: members up to it need one launch, larger
// ones log2(ceil(n / tile)) merge passes through global memory and a last launch that writes order / kept
uint32_t rank_tile(uint32_t max_n);
// the single form (the arguments travel as kernel arguments) and the grouped one (member = blockIdx.z, device-visible table)
hipError_t launch_rank(const RankArgs &args, hipStream_t stream);
hipError_t launch_rank_g(const RankArgs *tab, uint32_t G, uint32_t max_n, hipStream_t stream);
// k_ingest / k_ingest_g reading row order[j] into output row j, j < *kept (both device-resident: no host round trip between the
// ranking and the copy); n: the rows of the source, the upper bound of *kept.  Both sets are always written.
struct IngestRankedArgs {
    IngestSrc a, b;
    uint32_t n, pad;
    const uint32_t *order, *kept;
    double *out_a, *out_b;
};
hipError_t launch_ingest_ranked(const IngestRankedArgs &args, hipStream_t stream);
hipError_t launch_ingest_ranked_g(const IngestRankedArgs *tab, uint32_t G, uint32_t max_n, hipStream_t stream);
// After the LM kernels: records of the refined models on the device (skipped tasks keep their input record), and the
// choice "refined model if its score beats `incumbent_score`, else the incumbent" of the final refinement
// (ransac_impl.h:190-198) so that the inlier mask can follow without a host round trip.
// host_tasks (pinned host memory, may be null): receives params / skipped / iterations / costs of every task
hipError_t launch_task_records(int est, const LMTask *tasks, const double *records_in, double *records_out,
                               uint32_t num_tasks, LMTask *host_tasks, hipStream_t stream);
hipError_t launch_select_record(const double *score_refined, double incumbent_score, const double *rec_refined,
                                const double *rec_incumbent, double *out, hipStream_t stream);
// rows of the correspondence operand table of k_score_mfma for n points (chunks x points per chunk of its launch)
uint32_t abs16_point_rows(uint32_t n_points);
bool score_uses_mfma(int est, uint32_t n_points, const PrefilterArgs &pf);
// operands of k_score_mfma2 for `capacity` hypotheses listed in `slots` (+ the pad rows behind them)
hipError_t launch_sampson16(BatchCtl *ctl, const uint32_t *slots, const double *models, uint32_t capacity, void *out,
                            hipStream_t stream);
// operands of k_score_mfmah for `capacity` hypotheses listed in `slots` (the last group of 8 is filled up)
hipError_t launch_hom16(BatchCtl *ctl, const uint32_t *slots, const double *models, uint32_t capacity, float thr, void *out,
                        hipStream_t stream);
size_t lm2_state_bytes(uint32_t num_tasks);
size_t lm2_partial_bytes(uint32_t num_tasks, uint32_t slices);
hipError_t launch_lm2(int est, const PointSet &pts, LMTask *tasks, uint32_t num_tasks, uint32_t slices,
                      uint32_t max_iterations, bool loss_changes, void *states, double *partials, hipStream_t stream);
// chunks = ceil(n / (kScoreThreads * P)); P is chosen inside from n (returned through *chunks_out)
uint32_t score_chunks(int est, uint32_t n_points, bool prefilter, bool mfma = false);
int score_points_per_lane(int est, uint32_t n_points, bool streaming, bool mfma); // ... and the P that goes with the chunks
// most hypothesis slices (workgroups per chunk) launch_score gives a streaming launch of `chunks` chunks
uint32_t score_slice_limit(int est, uint32_t chunks, bool mfma);
// slices: workgroups of kScoreThreads per chunk; the streaming kernels run 8 wavefronts per workgroup, i.e. slices / 2 of them
hipError_t launch_score(int est, const ScoreArgs &a, uint32_t slices, hipStream_t stream);
// absolute pose on the matrix cores with a.prune set: lead, survivor counts, pre-selection, exact scores; launch_prune_lead / launch_prune_select
// are the two small steps between the scorer launches
hipError_t launch_score_pruned(const ScoreArgs &a, uint32_t slices, hipStream_t stream);
// diagnostic entries: the filter's counts alone, whole list and every chunk, and the exact rule's label of the pre-selected positions
hipError_t launch_score_count(const ScoreArgs &a, uint32_t slices, hipStream_t stream);
hipError_t launch_prune_label(const ScoreArgs &a, hipStream_t stream);
hipError_t launch_prune_lead(const ScoreArgs &a, hipStream_t stream);
hipError_t launch_prune_select(const ScoreArgs &a, hipStream_t stream);
int tangent_score_chunk(); // correspondences per chunk of k_score_tangent (EST_RELT)
int radial1d_score_chunk(); // correspondences per chunk of k_score_radial1d (EST_RAD1D)
// num_models[iters] -> slots (compact list of record indices in (iteration, model) order) + count
hipError_t launch_lm(int est, const PointSet &pts, LMTask *tasks, uint32_t num_tasks, hipStream_t stream);
// An inlier mask's destination in the CALLER's device memory (pl_device_mask once the driver has checked it): the flag of the
// run's row i goes to byte (order ? order[i] : i) * stride - order: the permutation a scored item's ranking left in device
// memory (rank.hip), so the flags land in the caller's numbering without a host round trip.  data == null: none.
struct MaskDest {
    uint8_t *data;
    int64_t stride; // BYTES between the flags of consecutive rows, >= 1
    const uint32_t *order;
};
// host_mask (pinned, device-mapped; may be null): the kernel writes a second copy there itself - no copy dispatch
// dst (may be null): ... and the caller's device copy, in the same launch
hipError_t launch_mask(int est, const PointSet &pts, const double *model, double thr2, uint8_t *mask,
                       uint8_t *host_mask, hipStream_t stream, const MaskDest *dst = nullptr);
// Zero flags for the n rows of every member's destination (ingest.hip): what a destination holds for the rows its scores drop and
// for an item whose host form writes no mask.  member = blockIdx.z, device-visible table; max_n: the largest n of the table
struct MaskFillArgs {
    uint8_t *data;
    int64_t stride;
    uint32_t n, pad;
};
hipError_t launch_mask_fill_g(const MaskFillArgs *tab, uint32_t G, uint32_t max_n, hipStream_t stream);

// ---- device-side bookkeeping (pipeline.hip) ----
// the fp16 operand blocks of the matrix-core scorers, built in the same launch as the hypothesis-ordered copies (see
// k_gather_shadow16); out == nullptr: none
struct Shadow16Params {
    void *out = nullptr;
    float g16 = 0.f, c16 = 0.f, thr = 0.f;
    int sampson = 0; // 1: two-view, operands of k_score_mfma2 (96 B per hypothesis, pl_prefilter.h Sampson16Operand);
                     // 2: homography, operands of k_score_mfmah (256 B per hypothesis, Hom16Model; thr = PrefilterArgs.h16)
    // absolute pose (sampson == 0, k_score_mfma) only.  The operand rows in `out` are those of the LIVE hypotheses, indexed by
    // live position; k_compact2 writes the list and its inverse:
    uint32_t *live = nullptr;   // [capacity] record index of the live hypotheses, ascending hypothesis index
    uint32_t *rank = nullptr;   // [capacity] hypothesis k -> live position or kNoRank
    const uint32_t *nan_bits = nullptr; // optional [iterations]: the generator's NaN flags per iteration (GenerateArgs.nan_bits);
                                // nullptr: k_compact2 reads the flag word of every record
    void *points16 = nullptr;   // [point_rows] operand rows of the correspondences, rebuilt by every launch that builds `out`
    uint32_t point_rows = 0;    // chunks x correspondences per chunk (rows past the last correspondence: invalid columns)
};
constexpr size_t kSampson16Bytes = 96;
constexpr size_t kAbs16Bytes = 64;  // absolute pose (k_score_mfma): 3 directions + the shared second k block, 16 B each, per hypothesis
constexpr size_t kAbs16Pad = 32;    // the last group of 32 (of the live list) is filled up
constexpr size_t kAbs16PointBytes = 64; // ... and per correspondence: first k block + the second k block of the 3 directions
constexpr size_t kSampson16Pad = 64; // operand rows a partial group of 32 may read past the last hypothesis
constexpr size_t kHom16Bytes = 256; // homography (k_score_mfmah): 4 rows x 4 k blocks x 16 B per hypothesis, groups of 8
constexpr size_t kHom16Pad = 8;     // the last group of 8 is filled up
// Everything k_score_mfma needs for `capacity` hypotheses that sit in `models` in list order `slots` (diagnostic entry
// pl_debug_score_stream; the main loop gets the same from launch_compact2): live list + rank + ctl->num_live, the operand rows
// of the live hypotheses and of the correspondences (all fields of s16 set).
hipError_t launch_abs16(BatchCtl *ctl, const uint32_t *slots, const double *models, uint32_t capacity, const PointSet &pts,
                        const Shadow16Params &s16, hipStream_t stream);
// the two halves on their own (diagnostic entry pl_debug_score_stream): hypothesis-ordered copies of records that already
// sit in `models` in list order `slots`, and the chunk partials -> (count, score) without the record scan
hipError_t launch_gather_models(BatchCtl *ctl, const uint32_t *slots, const double *models, uint32_t capacity,
                                float *shadow_compact, double *compact64, hipStream_t stream);
hipError_t launch_finalize(const FinalizeArgs &f, hipStream_t stream);

// ---- groups of problems: one launch sequence for MANY independent problems (BASELINE config 4) ----------------------
// The problem index is a grid dimension (blockIdx.z) and every kernel fetches its arguments from a device-resident
// table with one entry per problem of the group - the same kernel bodies as the single-problem launches above, so a
// batch of 64 default-option problems costs the ~10 launches of one problem instead of 64 x 10.
struct SampleArgs {
    uint64_t seed, pos_base, N;
    uint32_t B, M;
    uint8_t *delta;
    uint64_t *flagbits; // >= ceil(M / 64) words
    uint32_t *positions;
    BatchCtl *ctl;
    uint32_t zero_words, pad; // zero_words: 32-bit words starting at `ctl` (control block + the tables behind it) that the
                              // first kernel zeroes itself (0: the caller has done it)
};
struct CompactArgs {
    const uint32_t *num_models;
    uint32_t B;
    int32_t maxm;
    uint32_t *blk_tot, *slots, *offsets; // blk_tot is followed by the generators' NaN-model table (ceil(B / 1024) + 1 entries each)
    const double *models;
    float *shadow;
    double *compact64;
    BatchCtl *ctl;
    Shadow16Params s16;
    uint32_t *host_offsets; // optional pinned mirror of `offsets` (the host needs offsets[stop] after its replay)
};
struct RecordsArgs {
    FinalizeArgs f;
    const uint32_t *slots;
    const double *models;
    uint32_t *blk_max;
    double *blk_min;
    uint32_t init_max, rec_cap;
    double init_min;
    RecordMeta *rec_meta;
    double *rec_models;
    BatchCtl *ctl;
    RecordMeta *host_meta;
    double *host_models;
    uint32_t host_cap, pad;
};
// The single-problem forms of the three launches (the other kernels of a batch step: launch_generate, launch_score,
// launch_score_seq).  counted: blk_tot already holds the per-block model counts (GenerateArgs.blk_tot), otherwise they are
// counted first; pts: the problem's correspondences (read where s16.points16 is set)
// build (host side, diagnostics): 0 = the orbit kernel's build as orbit_small_build picks it, 1 = the small build, 2 = the large one
hipError_t launch_sample_positions(int K, const SampleArgs &a, hipStream_t stream, int build = 0);
// ... and the orbit walk alone, over a delta table and a bitmap that are in place (pl_debug_sample_positions plants them)
hipError_t launch_sample_orbit(int K, const SampleArgs &a, hipStream_t stream, int build = 0);
// The orbit kernel's two builds: which one a window of M positions over N correspondences takes, and what each holds - flagged
// positions, the most of them pointer doubling follows (more: the one-lane walk), segments - and the positions of a phase-1 tile.
bool orbit_small_build(uint32_t M, uint64_t N, int K);
struct OrbitShape {
    uint32_t flags, doubling, segments, tile;
};
OrbitShape orbit_build_shape(bool small);
hipError_t launch_compact2(const CompactArgs &a, bool counted, const PointSet &pts, hipStream_t stream);
hipError_t launch_finalize_records(const RecordsArgs &a, hipStream_t stream);
struct MaskArgs {
    PointSet pts;
    const double *model;
    double thr2;
    uint8_t *mask, *host_mask;
    MaskDest dst; // the caller's device copy (pl_estimate_batch_dev_masked); data == null: none
};
struct SelectArgs {
    const double *score_refined;
    double incumbent_score;
    const double *rec_refined, *rec_incumbent;
    double *out;
    const uint32_t *count_refined; // optional: inlier count of the refined model ...
    uint32_t count_incumbent;      // ... and of the incumbent; the chosen one goes to
    uint32_t pad;
    uint32_t *count_out;           // ... this device word (gate of the tasks enqueued behind the choice)
    const uint32_t *fetch_src; // optional: one device word (a stopped problem's hypothesis offset) ...
    uint32_t *fetch_dst;       // ... copied to this (pinned host) address by the same launch
};
struct GroupArgs { // everything the kernels of one batch step need for ONE problem: an entry of a group's table, or the
                   // arguments of the single-problem launches (filled by wire_batch_step, driver.cc)
    uint32_t active;   // 0: the slot takes no part in this step
    uint32_t use_mfma; // absolute pose: scored by k_score_mfma (otherwise k_score_queue)
    uint32_t chunks, slices;
    SampleArgs samp;
    GenerateArgs gen;
    CompactArgs comp;
    ScoreArgs score;
    RecordsArgs rec;
    SeqScoreArgs seq;
};
// chunk = 64 * this many correspondences for two-view problems scored by k_score_mfma2 in a group (score_shape's bound)
constexpr int group_mfma2_points_per_lane(int est) { return est == EST_REL ? 5 : 6; }
struct GroupDims { // grid extents: maxima over the active problems of the group
    uint32_t G;          // problems (grid.z)
    uint32_t max_M;      // sampler window
    uint32_t min_n;      // fewest correspondences (most sample redraws: sizes the orbit kernel's tables)
    uint32_t max_B;      // iterations per batch
    uint32_t max_hcap;   // hypothesis slots
    uint32_t max_chunks, max_slices;
    uint32_t any_mfma, any_queue;
    uint32_t any_prune;  // a member's matrix-core scorer prunes (ScoreArgs.prune.st): the step launches lead, counts, pre-selection and exact scores
    uint32_t any_bound;  // ... and a pruning member runs the bound tier between pre-selection and exact scores (PruneArgs.bound)
    int P;               // points per lane of the scorers (chunk = 64 P correspondences)
};
// positions -> generate -> compact/gather(/fp16 operands) -> score -> finalize/records -> candidates re-scored: the
// whole batch step of every active problem of the group, one launch per kernel
// ev0 / ev1 (optional): recorded around the scoring launch(es)
hipError_t launch_group_batch(int est, const GroupArgs *args, const GroupDims &dims, hipStream_t stream,
                              hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
// the scorer launch(es) of the step on their own: matrix-core members (d.any_mfma) and fp32-queue members (d.any_queue) of the
// table, on a grid of (d.max_slices, d.max_chunks, d.G); workgroups beyond a member's own slices or chunks return
hipError_t launch_group_score(int est, const GroupArgs *args, const GroupDims &d, hipStream_t stream);
// ... and the two small steps between the scorer launches of a pruned step (d.any_prune; launch_prune_lead / launch_prune_select)
hipError_t launch_group_prune_lead(const GroupArgs *args, const GroupDims &d, hipStream_t stream);
hipError_t launch_group_prune_select(const GroupArgs *args, const GroupDims &d, hipStream_t stream);
hipError_t launch_group_score_count(const GroupArgs *args, const GroupDims &d, hipStream_t stream);
hipError_t launch_group_score_seq(int est, const SeqScoreArgs *args, uint32_t G, uint32_t max_cap, hipStream_t stream);
hipError_t launch_group_select(const SelectArgs *args, uint32_t G, hipStream_t stream);
hipError_t launch_group_mask(int est, const MaskArgs *args, uint32_t G, uint32_t max_n, hipStream_t stream);
struct PrepareGroupArgs {
    const double *a_raw, *b_raw;
    uint32_t n, pad;
    PrepareArgs args;
    double *soa;
    unsigned long long *absmax_bits;
    // optional (null: args.scale as ever): the member's record of a k_point_stats_g launch in front of this one on the same stream -
    // the kernel takes args.scale from stats->scale, so the host need not read the record back between the two launches
    const PointStatsRecord *stats;
};
hipError_t launch_group_prepare(const PrepareGroupArgs *args, uint32_t G, uint32_t max_n, hipStream_t stream);
// (pieces of launch_group_batch that live in pipeline.hip)
hipError_t launch_group_positions(int K, const GroupArgs *args, const GroupDims &d, hipStream_t stream, int build = 0); // (build: launch_sample_positions)
hipError_t launch_group_orbit(int K, const GroupArgs *args, const GroupDims &d, hipStream_t stream, int build = 0);     // the orbit walk alone
hipError_t launch_group_compact(const GroupArgs *args, const GroupDims &d, hipStream_t stream);
hipError_t launch_group_finalize_records(const GroupArgs *args, const GroupDims &d, hipStream_t stream);
// LM over the tasks of many problems: every task carries its own correspondences (LMTask.pts)
hipError_t launch_lm_tasks(int est, LMTask *tasks, uint32_t num_tasks, uint32_t max_points, hipStream_t stream);
// Summation order of the refinements.  0 (default): k_lm - reference order up to 256 correspondences, tree beyond - for poses and
// homographies, k_lm_ordered for fundamental matrices (the sign of a refined F hangs on the bits of its input, pl_svd3.h);
// 1: k_lm_ordered for every estimator; 2: k_lm for every estimator
void set_lm_mode(int mode);
int get_lm_mode();
bool lm_sums_ordered(int est); // what launch_lm_tasks will pick for this estimator
void set_lm_force_ordered(int on); // this host thread's LM launches in the reference's order whatever the mode (0: back to the mode)
// absolute pose + camera intrinsics (lm_cam.hip): tasks with cam_flags != 0; refined pose -> params / record_out, camera -> cam
hipError_t launch_lm_cam(LMTask *tasks, uint32_t num_tasks, hipStream_t stream);
int group_points_per_lane(int est); // P of the group launches (fixed per estimator)

// Bare solver entry points (one problem per lane); inputs/outputs in HBM.
//   abs : in = [x0 x1 x2 X0 X1 X2] (18 doubles / problem) -> out records (4 / problem)
hipError_t launch_solve_batch(int est, const double *in, uint32_t num_problems, double *models, uint32_t *num_models,
                              hipStream_t stream);

} // namespace pl
