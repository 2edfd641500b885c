// poselib_amd — host driver behind the C-ABI (include/poselib_amd.h).
//
// What runs where
//   device : sampler positions (k_sample_delta / k_sample_orbit), sample draw + minimal solve (k_generate, k_rel_*),
//            hypothesis scoring (k_score_mfma / k_score_queue), the running-best scan (k_finalize2 / k_records), the
//            decision-relevant scores in the reference's summation order (k_score_seq), all LM refinements
//            (k_lm / k_lm2), final inlier masks (k_mask), the per-point pre-processing of the front-ends (k_prepare).
//   host   : the sequential bookkeeping of LO-RANSAC (RansacRun), replayed over the device results so that the outcome
//            equals the reference's single-threaded loop (PoseLib/robust/ransac_impl.h:106-201):
//              pass 1  the candidate list of a batch - hypotheses that improve the running (inlier count, MSAC score)
//                      in (iteration, model) order - through the exact rule; best_minimal_* depends on minimal models
//                      only (:113-123), so the iterations that trigger LO and their seeds are known without LO results;
//              device  all triggered LOs of the batch run as ONE batched LM launch, then are re-scored;
//              pass 2  replay stats.model_score / best_model / dynamic_max_iter and the stop rule (:182)
//                      iteration by iteration; iterations evaluated past the stop are discarded.
//            plus, of the front-ends (PoseLib/robust.cc:36-126, 242-314, 544-594, 712-757), the two order-dependent
//            reductions of normalize_points, threshold rescaling and de-normalisation; PROSAC's serial sample schedule.
// There is no CPU fallback for any device stage: without a HIP device the entry points fail.
#include "../../include/poselib_amd.h"
#include "pl_focal.h"
#include "pl_kernels.h"
#include "pl_ranges.h"
#include "pl_refine_cam.h"
#include "pl_sfocal.h"
#include "pl_solver_6ptf.h"
#include "pl_solver_p35pf.h"
#include "pl_sampler.h"
#include "pl_svd3.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

using namespace pl;

namespace {

thread_local std::string g_err;

int fail(int code, const char *what, hipError_t e = hipSuccess) {
    g_err = what;
    if (e != hipSuccess) {
        g_err += ": ";
        g_err += hipGetErrorString(e);
    }
    return code;
}

#define HIP_TRY(expr)                                                                                                  \
    do {                                                                                                               \
        hipError_t _e = (expr);                                                                                        \
        if (_e != hipSuccess)                                                                                          \
            return fail(PL_ERR_HIP, #expr, _e);                                                                        \
    } while (0)

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap)
            return hipSuccess;
        if (p)
            (void)hipFree(p);
        p = nullptr;
        cap = 0;
        const size_t want = bytes + bytes / 4 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess)
            cap = want;
        return e;
    }
    template <typename T> T *as() const { return static_cast<T *>(p); }
};
struct HostBuf { // pinned and mapped: kernels write their small results here themselves (no copy dispatch); the
                 // host reads them after the stream synchronisation that follows
    void *p = nullptr;
    void *dp = nullptr; // the same memory as the device addresses it
    size_t cap = 0;
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap)
            return hipSuccess;
        if (p)
            (void)hipHostFree(p);
        p = dp = nullptr;
        cap = 0;
        const size_t want = bytes + bytes / 4 + 256;
        hipError_t e = hipHostMalloc(&p, want, hipHostMallocMapped);
        if (e != hipSuccess)
            return e;
        e = hipHostGetDevicePointer(&dp, p, 0);
        if (e != hipSuccess) {
            (void)hipHostFree(p);
            p = dp = nullptr;
            return e;
        }
        cap = want;
        return hipSuccess;
    }
    template <typename T> T *as() const { return static_cast<T *>(p); }
    template <typename T> T *dev() const { return static_cast<T *>(dp); }
};

struct Context {
    int device = -1;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // batch scratch
    DevBuf positions, samples, shadow16, lm2_states, lm2_partials, raw_a, raw_b, pts_arena, absmax, models, num_models, nan_bits, slots, num_hyp, part_count, part_score, count, score;
    DevBuf shadow, compact64;
    DevBuf prune_sel, prune_kept, prune_state; // pruned scoring of the live list (PruneArgs)
    DevBuf live, rank, points16; // k_score_mfma: live hypothesis list, its inverse, operand rows of the correspondences
    DevBuf offsets, ctl, blk_best, rec_meta, rec_models, delta, flags;
    DevBuf gen_stage; // workspace of the staged 5-point generator
    DevBuf iota; // iota[i] = i: a device-resident "number of hypotheses" for launches whose count the host knows
    DevBuf lm_tasks, lm_records, gather_idx, gather_out, mask, lm_scratch, tmp_model, solve_in, solve_out, solve_cnt, focal_stage;
    HostBuf h_rec_meta, h_focal, h_in;
    HostBuf h_pstats; // the record k_point_stats writes (the *_dev front-ends)
    HostBuf h_undistort; // the member table of pl_undistort_points_batch_dev
    HostBuf h_mask_fill; // ... and of the zero fill in front of a call with device masks (launch_mask_fill_g)
    // scored items (the *_dev_scored front-ends): the sides of the merge passes, the permutations, the permuted fp64 blocks; the
    // argument tables and the kept counts the kernels write
    DevBuf rank_keys, rank_rows, rank_order, ranked_pts;
    HostBuf h_rank, h_rank_order;
    const double *raw_src_a = nullptr, *raw_src_b = nullptr; // where the raw correspondences of the last make_problem_prepared live (device-visible)
    HostBuf h_absmax, h_positions, h_num_models, h_count, h_score, h_tasks, h_gather_idx, h_gather_out, h_mask,
        h_small, h_models;
};

constexpr uint32_t kIotaEntries = 4097;
thread_local Context *g_ctx = nullptr;

thread_local int g_requested_device = 0;
thread_local const pl_shard *g_shard = nullptr; // set around ransac_core by pl_ransac_run_sharded
// set around a single-problem *_dev run whose inlier mask goes to the caller's device memory (run_item_dev, driver_batch.inc): the
// launches that compute the returned model's mask write it there as well (RansacRun::run); the run's host `inliers` is then null
thread_local const MaskDest *g_mask_dest = nullptr;

int get_context(Context **out) {
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(PL_ERR_NO_DEVICE, "no HIP device available (poselib_amd has no CPU fallback)", e);
    if (g_ctx && g_ctx->device == g_requested_device) {
        HIP_TRY(hipSetDevice(g_ctx->device));
        *out = g_ctx;
        return PL_OK;
    }
    if (g_requested_device < 0 || g_requested_device >= ndev)
        return fail(PL_ERR_INVALID, "device index out of range");
    // (a context bound to another device is simply leaked for the lifetime of the thread)
    {
        // the kernels are built for gfx950 only (k_sample_orbit's large build alone keeps ~140 KB of static LDS): say so instead of
        // failing with "invalid device function" at the first launch
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, g_requested_device));
        if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
            static thread_local std::string msg;
            msg = std::string("device architecture ") + prop.gcnArchName +
                  " is not supported: poselib_amd is built for gfx950 (MI355X) only";
            return fail(PL_ERR_UNSUPPORTED, msg.c_str());
        }
    }
    struct Guard { // releases a half-built context on the failure paths
        Context *c;
        ~Guard() {
            if (!c)
                return;
            if (c->ev0)
                (void)hipEventDestroy(c->ev0);
            if (c->ev1)
                (void)hipEventDestroy(c->ev1);
            if (c->stream)
                (void)hipStreamDestroy(c->stream);
            if (c->iota.p)
                (void)hipFree(c->iota.p);
            delete c;
        }
    } guard{new Context()};
    Context *c = guard.c;
    c->device = g_requested_device;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreate(&c->ev0));
    HIP_TRY(hipEventCreate(&c->ev1));
    {
        std::vector<uint32_t> iota(kIotaEntries);
        for (uint32_t i = 0; i < kIotaEntries; ++i)
            iota[i] = i;
        HIP_TRY(c->iota.ensure(sizeof(uint32_t) * kIotaEntries));
        HIP_TRY(hipMemcpy(c->iota.p, iota.data(), sizeof(uint32_t) * kIotaEntries, hipMemcpyHostToDevice));
    }
    guard.c = nullptr;
    g_ctx = c;
    *out = c;
    return PL_OK;
}

// The HIP runtime multiplexes a process's streams onto GPU_MAX_HW_QUEUES hardware queues (4 by default), and kernels of streams
// that share a queue run one after the other.  The batch entry points keep 8 ... 16 launch chains in flight, one stream each: with
// the default, three of eight streams shared a queue and ran at half the rate of the two that had one to themselves
// (profiles/r04_batch_chain_4_queues.md; pl_estimate_batch 59.8 k -> 68 k problems/s).  The variable is read when the runtime
// initialises, i.e. at the process's first HIP call, and it belongs to the HOST APPLICATION: this library does not touch the
// process environment (round 4 set it from a constructor).  poselib_amd/_lib.py (the Python binding), bench.py and
// the reference-side binding's documentation set / recommend GPU_MAX_HW_QUEUES=16.

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// POSELIB_AMD_GROUP_TIMING=1 (diagnostic): pl_estimate_batch reports where its workers' time went - waiting for the device,
// in the per-item preparation, in fallback items - on stderr
std::atomic<uint64_t> g_t_wait_ns{0}, g_t_group_ns{0}, g_t_prep_ns{0}, g_t_fallback_ns{0}, g_n_waits{0}, g_n_fallback{0};
const bool g_group_timing = std::getenv("POSELIB_AMD_GROUP_TIMING") != nullptr;
// host work a worker of pl_estimate_batch does INSTEAD of idling at its next wait (staging the next group's inputs); one shot
thread_local std::function<void()> g_wait_hook;
thread_local std::vector<double> g_wait_marks; // (diagnostic) end of every wait of this worker's current job, seconds
// Wait for everything enqueued on the context's stream.
hipError_t wait_stream(Context *c) {
    if (g_wait_hook) {
        std::function<void()> h;
        h.swap(g_wait_hook);
        h();
    }
    if (!g_group_timing)
        return hipStreamSynchronize(c->stream);
    const double t0 = now_s();
    const hipError_t e = hipStreamSynchronize(c->stream);
    const double t1 = now_s();
    g_t_wait_ns += (uint64_t)((t1 - t0) * 1e9);
    ++g_n_waits;
    g_wait_marks.push_back(t0);
    g_wait_marks.push_back(t1);
    return e;
}

} // namespace

struct pl_problem {
    int kind;
    int device;
    uint32_t n;
    double *d_pts; // SoA block: nd arrays of n doubles
    PointSet ps;
    bool borrowed = false; // d_pts lives in the calling thread's context arena (one-shot front-ends): not freed
};

namespace {

LMOptions to_lm(const pl_bundle_options &b) {
    LMOptions o;
    o.max_iterations = (uint32_t)std::min<uint64_t>(b.max_iterations, 0xffffffffu);
    o.loss_type = b.loss_type;
    o.lambda_update = b.lambda_update;
    o.damping = b.damping;
    o.loss_scale = b.loss_scale;
    o.gradient_tol = b.gradient_tol;
    o.step_tol = b.step_tol;
    o.relative_cost_tol = b.relative_cost_tol;
    o.initial_lambda = b.initial_lambda;
    o.min_lambda = b.min_lambda;
    o.max_lambda = b.max_lambda;
    o.lambda_factor = b.lambda_factor;
    return o;
}
// bundle.refine_* as CamRefineFlags, reduced to the flags that select at least one parameter of the model (0: the pose alone,
// k_lm's case)
int active_cam_flags(int model_id, const pl_bundle_options &b) {
    const int flags = (b.refine_focal_length ? CAM_REFINE_FOCAL : 0) | (b.refine_principal_point ? CAM_REFINE_PRINCIPAL : 0) |
                      (b.refine_extra_params ? CAM_REFINE_EXTRA : 0);
    int idx[kCamMaxParams];
    return camera_refinement_idx(model_id, flags, idx) > 0 ? flags : 0;
}
LMOptions lo_options(double max_error) { // estimators/absolute_pose.cc:61-64 (identical in the four estimators)
    pl_bundle_options b;
    pl_default_bundle_options(&b);
    b.loss_type = LOSS_TRUNCATED;
    b.loss_scale = max_error;
    b.max_iterations = 25;
    return to_lm(b);
}
CameraParams to_cam(const pl_camera *c) {
    CameraParams r;
    std::memset(&r, 0, sizeof(r));
    if (!c) {
        r.model_id = CAM_NULL;
        return r;
    }
    r.model_id = c->model_id;
    r.num_params = c->num_params;
    for (int i = 0; i < 12; ++i)
        r.p[i] = c->params[i];
    return r;
}
// The fisheye models take EXACTLY their parameter count: the reference's inverse (undistort_theta_poly, camera_models.cc:613-662) reads
// every parameter from the first coefficient to params.size() as a further coefficient of the polynomial in theta, while its projection
// reads the model's own - with more parameters than the model has, un-projection is no longer the inverse of projection.
bool camera_supported(const pl_camera *c) {
    return c->model_id == CAM_NULL || (c->model_id == CAM_SIMPLE_PINHOLE && c->num_params >= 3) ||
           (c->model_id == CAM_PINHOLE && c->num_params >= 4) || (c->model_id == CAM_SIMPLE_RADIAL && c->num_params >= 4) ||
           (c->model_id == CAM_RADIAL && c->num_params >= 5) || (c->model_id == CAM_OPENCV && c->num_params >= 8) ||
           (c->model_id == CAM_OPENCV_FISHEYE && c->num_params == 8) || (c->model_id == CAM_SIMPLE_RADIAL_FISHEYE && c->num_params == 4) ||
           (c->model_id == CAM_RADIAL_FISHEYE && c->num_params == 5);
}
double camera_focal(const pl_camera *c) { // misc/camera_models.cc:304-323
    if (c->num_params == 0)
        return 1.0;
    switch (c->model_id) {
    case CAM_SIMPLE_PINHOLE:
    case CAM_SIMPLE_RADIAL:
    case CAM_RADIAL:
    case CAM_SIMPLE_RADIAL_FISHEYE:
    case CAM_RADIAL_FISHEYE:
        return 0.0 + c->params[0] / 1;
    case CAM_PINHOLE:
    case CAM_OPENCV:
    case CAM_OPENCV_FISHEYE:
        return 0.0 + c->params[0] / 2 + c->params[1] / 2;
    default:
        return 1.0;
    }
}
void camera_set_focal(pl_camera *c, double f) { // misc/camera_models.cc:96-107 over the model's focal_idx
    if (camera_has_two_focals(c->model_id) && c->num_params >= 2) {
        c->params[0] = f;
        c->params[1] = f;
    } else if (c->model_id != CAM_NULL && !camera_has_two_focals(c->model_id) && c->num_params >= 1) {
        c->params[0] = f;
    }
}
void camera_rescale(CameraParams &c, double s) { // misc/camera_models.cc:432-455
    if (c.num_params == 0)
        return;
    if (c.model_id != CAM_NULL && !camera_has_two_focals(c.model_id)) { // (the distortion parameters stay)
        c.p[0] *= s, c.p[1] *= s, c.p[2] *= s;
    } else if (camera_has_two_focals(c.model_id)) {
        for (int i = 0; i < 4; ++i)
            c.p[i] *= s;
    }
}

// ---- model <-> parameter block <-> record conversions (host side, IEEE add/mul only) ----
// `model` is the user-facing representation: pose = 7 doubles (q,t); matrix = 9 doubles ROW-major here.
void params_from_record(int kind, const double *rec, double *params) {
    for (int i = 0; i < kParamDoubles; ++i)
        params[i] = 0.0;
    if (kind == EST_ABS || kind == EST_REL || kind == EST_RELT || kind == EST_RAD1D) {
        for (int i = 0; i < 7; ++i)
            params[i] = rec[i];
    } else {
        for (int i = 0; i < 9; ++i)
            params[i] = rec[kMatOff + i];
    }
}

// Parameter block that enters k_lm for a model given as record.
void lm_params_from_record(int kind, const double *rec, double *params) {
    params_from_record(kind, rec, params);
    if (kind == EST_FUND) { // factorise F = U diag(1, sigma, 0) V^T  (bundle.cc:318-319)
        Mat3 F;
        for (int i = 0; i < 9; ++i)
            F.m[i] = rec[kMatOff + i];
        for (int i = 0; i < kParamDoubles; ++i)
            params[i] = 0.0;
        fundamental_lm_params(F, params);
    }
}
void identity_record(int kind, double *rec) {
    if (kind == EST_ABS || kind == EST_REL || kind == EST_RELT || kind == EST_RAD1D) {
        Quat q;
        q.w = 1.0, q.x = q.y = q.z = 0.0;
        store_pose_model_q(rec, q, v3(0, 0, 0), kind == EST_REL || kind == EST_RELT);
    } else {
        Mat3 I;
        for (int i = 0; i < 9; ++i)
            I.m[i] = (i % 4 == 0) ? 1.0 : 0.0;
        store_matrix_model(rec, I);
    }
}

// ---- iteration bound (ransac_impl.h:43-73) ----
double prob_all_inliers(uint64_t inl, uint64_t N, uint64_t K) {
    if (K == 0)
        return 1.0;
    if (inl < K || N < K)
        return 0.0;
    double p = 1.0;
    for (uint64_t i = 0; i < K; ++i)
        p *= static_cast<double>(inl - i) / static_cast<double>(N - i);
    return p;
}
uint64_t dynamic_max_iter(uint64_t inl, uint64_t N, uint64_t K, double log_fail, double mult, uint64_t min_it,
                          uint64_t max_it) {
    const double p = prob_all_inliers(inl, N, K);
    if (p >= 0.9999)
        return min_it;
    if (p <= 0.0001)
        return max_it;
    // The reference converts the double to size_t with a plain static_cast (ransac_impl.h:70-71), which is undefined
    // for values that do not fit - success_prob = 1 gives log(0) = -inf and hence +inf here.  Its de-facto behaviour
    // (gcc, x86-64: cvttsd2si on x - 2^63 and a sign-bit flip for x >= 2^63) is spelled out so that it does not depend
    // on the compiler of this file: +inf and everything >= 2^64 become 0, NaN becomes 2^63.
    const double v = std::ceil(log_fail / std::log(1.0 - p) * mult);
    const double two63 = 9223372036854775808.0;
    auto cvttsd2si = [&](double x) -> int64_t {
        return (x >= -two63 && x < two63) ? static_cast<int64_t>(x) : std::numeric_limits<int64_t>::min();
    };
    const uint64_t n = (v >= two63) ? (static_cast<uint64_t>(cvttsd2si(v - two63)) ^ 0x8000000000000000ull)
                                    : static_cast<uint64_t>(cvttsd2si(v));
    return std::max(min_it, std::min(max_it, n));
}

// Host replay of the sampler to find where each iteration's draws start (integer work, a few ns per
// draw): out[i] = draws consumed before iteration i, RELATIVE to `pos` (like the device's k_sample_orbit; the
// generators add GenerateArgs.pos_base).  Returns the absolute draw position after `count` iterations.
template <int K> uint64_t sample_positions(uint64_t seed, uint64_t pos, uint64_t N, uint32_t count, uint32_t *out) {
    uint32_t idx[K];
    const uint64_t pos0 = pos;
    for (uint32_t i = 0; i < count; ++i) {
        out[i] = (uint32_t)(pos - pos0);
        pos += draw_sample<K>(seed, pos, N, idx);
    }
    return pos;
}
uint64_t sample_positions_k(int K, uint64_t seed, uint64_t pos, uint64_t N, uint32_t count, uint32_t *out) {
    switch (K) {
    case 3:
        return sample_positions<3>(seed, pos, N, count, out);
    case 4:
        return sample_positions<4>(seed, pos, N, count, out);
    case 5:
        return sample_positions<5>(seed, pos, N, count, out);
    default:
        return sample_positions<7>(seed, pos, N, count, out);
    }
}

// PROSAC sampling (PoseLib/robust/sampling.cc:85-136): the size of the subset the sample is drawn from follows a
// serial recurrence over the iteration counter, so the samples of a batch are drawn on the host - one splitmix64
// draw (pl_sampler.h draw_at) per index - and handed to k_generate explicitly.  After max_prosac_iterations the
// sampler is the uniform one again (sampling.cc:101-102).
// (ProsacSampler: pl_sampler.h)

// Parameters of the scoring kernels' conservative fp32 pre-filters (pl_prefilter.h) for a problem.  Every value is rounded UP;
// POSELIB_AMD_NO_PREFILTER=1 disables the filters (exact evaluation of every point).
PrefilterArgs problem_prefilter(const pl_problem *p, double thr2) {
    static const bool disabled = std::getenv("POSELIB_AMD_NO_PREFILTER") != nullptr;
    PrefilterArgs pf = make_prefilter_args(p->kind, thr2, p->ps.xy_absmax);
    if (disabled)
        pf.enabled = 0;
    return pf;
}

// k_score_seq in plain mode: the `n` (< kIotaEntries) model records at `models` in the reference's summation order, results to
// count[] / score[] and to their pinned mirrors (written by the kernel itself)
SeqScoreArgs plain_seq_args(const Context *c, const PointSet &pts, const double *models, uint32_t n, double thr2, uint32_t *count,
                            double *score, uint32_t *host_count, double *host_score) {
    SeqScoreArgs q;
    q.pts = pts;
    q.models = models;
    q.cand = nullptr;
    q.num = c->iota.as<uint32_t>() + n; // the count is read from the device-resident table: no upload
    q.cap = n;
    q.thr2 = thr2;
    q.count = count, q.score = score;
    q.host_count = host_count, q.host_score = host_score;
    q.host_cand = nullptr;
    q.host_cap = 0;
    return q;
}

// Score `nrec` model records that already sit in device memory at `d_records`, in the reference's summation order
// (k_score_seq).  Results land in c->count / c->score and in the pinned h_count / h_score buffers after the caller
// synchronises.
int enqueue_score_records(Context *c, const pl_problem *p, const double *d_records, uint32_t nrec, double thr2) {
    HIP_TRY(c->num_hyp.ensure(sizeof(uint32_t)));
    HIP_TRY(c->count.ensure(sizeof(uint32_t) * nrec));
    HIP_TRY(c->score.ensure(sizeof(double) * nrec));
    HIP_TRY(c->h_count.ensure(sizeof(uint32_t) * nrec));
    HIP_TRY(c->h_score.ensure(sizeof(double) * nrec));
    SeqScoreArgs sa = plain_seq_args(c, p->ps, d_records, nrec, thr2, c->count.as<uint32_t>(), c->score.as<double>(),
                                     c->h_count.dev<uint32_t>(), c->h_score.dev<double>());
    if (nrec >= kIotaEntries) { // beyond the table: the count is uploaded
        HIP_TRY(hipMemcpyAsync(c->num_hyp.p, &nrec, sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        sa.num = c->num_hyp.as<uint32_t>();
    }
    HIP_TRY(launch_score_seq(p->kind, sa, c->stream));
    return PL_OK;
}

constexpr uint32_t kRecordCap = 1024;  // device record list capacity (overflow -> host scan fallback)
constexpr uint32_t kRecordFirst = 64;  // records fetched together with the control block

// ---- one batch step of ONE problem: positions -> generate -> compact/gather (+ fp16 operands) -> score -> finalize/records ->
// candidates re-scored.  The single-problem path (RansacRun::enqueue_batch: buffers of the Context, k_x launches) and the groups
// (run_group: slots of the arena, k_x_g launches over a table) size their buffers and build their kernel arguments HERE. ----
struct BatchShape {
    uint32_t B;          // iterations of the whole batch: the sampler walks all of them
    uint32_t lo, Bl;     // this rank's share [lo, lo + Bl) of them: everything from the generator on
    uint32_t M;          // the device sampler's window of draw positions (0: the positions come from the host)
    uint32_t slots;      // record slots per iteration
    uint32_t chunks;     // the scorer's chunks of correspondences
    uint32_t point_rows; // matrix-core absolute pose: rows of the correspondences' operand table
    bool use_mfma;       // scored on the matrix cores (score_uses_mfma)
    bool prune = false;  // matrix-core absolute pose: the step scores in two phases (score_prune_gate, driver_group.inc)
};
bool score_prune_gate(int kind, bool use_mfma, uint32_t iterations, uint32_t chunks); // (driver_group.inc, next to group_score_slices)
// The device sampler's window (BatchShape.M) for a batch of B iterations over N >= K correspondences: the draws an iteration is
// expected to consume (sum N / (N - i)), 5 % on top, and 8192 positions of slack.  The single run, a group's slot and every member
// of a group's step size their windows here, so no member of a full-size batch outgrows the slot.
uint64_t sampler_window(uint32_t N, int K, uint32_t B) {
    double per_it = 0;
    for (int i = 0; i < K; ++i)
        per_it += static_cast<double>(N) / static_cast<double>(N - (uint32_t)i);
    return (uint64_t)(B * per_it * 1.05) + 8192;
}
struct BatchSizes { // bytes of every device buffer of the step
    size_t positions, delta, flags, samples, models, num_models, nan_bits, slots, offsets, ctl, shadow, compact64, shadow16, live, rank,
        points16, part_count, part_score, count, score, blk_best, rec_meta, rec_models, gen_stage, prune_sel, prune_kept, prune_state;
};
struct BatchBuffers { // ... the buffers themselves, and where the kernels mirror their small results in pinned host memory
    uint32_t *positions, *samples /* explicit minimal samples of the share */, *num_models, *nan_bits, *slots, *offsets, *live, *rank;
    uint8_t *delta;
    uint64_t *flags;
    BatchCtl *ctl;
    float *shadow;
    double *models, *compact64, *part_score, *score, *rec_models;
    uint32_t *part_count, *count;
    RecordMeta *rec_meta;
    char *shadow16, *points16, *blk_best, *gen_stage;
    uint32_t *prune_sel; // pruned scoring (PruneArgs): the selection list, ...
    uint8_t *prune_kept; // ... kept / pruned per live position, ...
    char *prune_state;   // ... the PruneState and, 256 bytes behind it, the kept positions per tile of 1024
    RecordMeta *host_meta; // the first kRecordFirst candidates ...
    double *host_models;   // ... and their model records
    BatchCtl *host_ctl;    // the control block as the last kernel of the step finds it
};
// Behind the control block, zeroed with it: models and NaN models per 1024 iterations (two tables of nblk + 1 entries, filled by
// the generator), then the scorer's work counters (one per chunk of correspondences).
uint32_t batch_blocks(uint32_t Bl) { return (Bl + 1023) / 1024; }
size_t batch_ctl_bytes(uint32_t Bl, uint32_t chunks) {
    static_assert(sizeof(BatchCtl) % 4 == 0, "zeroed as 32-bit words");
    return sizeof(BatchCtl) + sizeof(uint32_t) * (2 * (size_t)batch_blocks(Bl) + 2 + chunks);
}
constexpr size_t kPruneTilesOffset = 256; // prune_state: the PruneState, from this offset the kept positions per tile
static_assert(sizeof(PruneState) <= kPruneTilesOffset, "prune_state layout");
constexpr size_t kBlkMinOffset = 1024; // blk_best: 256 running maxima (uint32_t), from this offset 256 running minima (double)

BatchSizes batch_step_sizes(int kind, const BatchShape &s) {
    const size_t iters = std::max<uint32_t>(s.Bl, 1u), hcap = iters * s.slots;
    // The live list, its inverse, the generator's NaN flags and the operand rows of the correspondences belong to the matrix-core
    // absolute-pose scorer alone; the other operand blocks to the matrix-core scorer of their kind.  A single run knows its scorer
    // and reserves them only then; a group packs one layout for all its members before any member's scorer is known and asks
    // with use_mfma = true: every absolute-pose member has them.
    const bool abs16 = s.use_mfma && kind == EST_ABS;
    BatchSizes z;
    z.positions = sizeof(uint32_t) * s.B;
    z.delta = (size_t)s.M + 64;
    z.flags = sizeof(uint64_t) * ((size_t)s.M / 64 + 2); // bitmap of redrawing positions
    z.samples = sizeof(uint32_t) * (size_t)s.B * sample_size(kind); // PROSAC: host-drawn samples [B][K]
    z.models = sizeof(double) * kModelStride * hcap;
    z.num_models = sizeof(uint32_t) * iters;
    z.nan_bits = abs16 ? sizeof(uint32_t) * iters : 0; // NaN flags per iteration (GenerateArgs.nan_bits)
    z.slots = sizeof(uint32_t) * hcap;
    z.offsets = sizeof(uint32_t) * iters;
    z.ctl = batch_ctl_bytes(s.Bl, s.chunks);
    z.shadow = sizeof(float) * 16 * hcap;
    z.compact64 = sizeof(double) * kModelDoubles * hcap;
    z.shadow16 = !s.use_mfma        ? 0
                 : kind == EST_ABS ? (hcap + kAbs16Pad) * kAbs16Bytes
                 : kind == EST_HOM ? (hcap + kHom16Pad) * kHom16Bytes
                                   : (hcap + kSampson16Pad) * kSampson16Bytes;
    z.live = z.rank = abs16 ? sizeof(uint32_t) * hcap : 0;
    z.points16 = abs16 ? kAbs16PointBytes * s.point_rows : 0;
    z.part_count = sizeof(uint32_t) * s.chunks * hcap;
    z.part_score = sizeof(double) * s.chunks * hcap;
    z.count = sizeof(uint32_t) * hcap;
    z.score = sizeof(double) * hcap;
    z.blk_best = kBlkMinOffset + sizeof(double) * 256;
    z.rec_meta = sizeof(RecordMeta) * kRecordCap;
    z.rec_models = sizeof(double) * kModelStride * kRecordCap;
    z.gen_stage = generate_stage_bytes(kind, s.Bl);
    // pruned scoring of the live list: reserved with the list (a group's slot serves steps that prune and steps that do not)
    z.prune_sel = abs16 ? sizeof(uint32_t) * hcap : 0;
    z.prune_kept = abs16 ? hcap : 0;
    z.prune_state = abs16 ? kPruneTilesOffset + sizeof(uint32_t) * ((hcap + 1023) / 1024) : 0;
    return z;
}

struct BatchRun { // the state of a run its next batch step starts from (RansacRun::batch_run)
    int kind;
    PointSet pts;
    uint64_t seed, pos; // pos: sampler draws consumed so far
    double thr2;
    PrefilterArgs pf;
    uint32_t init_max; // best_min_inl / best_min_score: what a candidate has to beat
    double init_min;
    int32_t real_focal_check;
    bool explicit_samples; // PROSAC: b.samples holds the share's samples
};

// Everything the kernels of the step need (GroupArgs: an entry of a group's table, or the arguments of the single-problem
// launches), except `slices` - the scorer's grid is the caller's choice.
void wire_batch_step(GroupArgs &a, const BatchRun &r, const BatchShape &s, const BatchBuffers &b) {
    std::memset(&a, 0, sizeof(a));
    const size_t hcap = (size_t)std::max<uint32_t>(s.Bl, 1u) * s.slots;
    const uint32_t nblk = batch_blocks(s.Bl);
    uint32_t *const blk_tot = reinterpret_cast<uint32_t *>(b.ctl + 1);
    const bool live_list = s.use_mfma && r.kind == EST_ABS; // k_score_mfma streams the hypotheses without a NaN entry
    a.active = 1;
    a.use_mfma = s.use_mfma ? 1u : 0u;
    a.chunks = s.chunks;
    // sampler (its first kernel clears the control block and the tables behind it)
    a.samp.seed = r.seed, a.samp.pos_base = r.pos, a.samp.N = r.pts.n, a.samp.B = s.B, a.samp.M = s.M;
    a.samp.delta = b.delta;
    a.samp.flagbits = b.flags;
    a.samp.positions = b.positions;
    a.samp.ctl = b.ctl;
    a.samp.zero_words = (uint32_t)(batch_ctl_bytes(s.Bl, s.chunks) / 4);
    // generator
    GenerateArgs &ga = a.gen;
    ga.pts = r.pts;
    ga.seed = r.seed;
    ga.pos_base = r.pos;
    ga.positions = b.positions + s.lo;
    ga.samples = r.explicit_samples ? b.samples : nullptr;
    ga.num_iters = s.Bl;
    ga.slots_per_iter = s.slots;
    ga.ctl = b.ctl;
    ga.models = b.models;
    ga.num_models = b.num_models;
    ga.real_focal_check = r.real_focal_check;
    ga.blk_tot = blk_tot;
    ga.blk_nan = blk_tot + nblk;
    ga.nan_bits = live_list ? b.nan_bits : nullptr; // the live list of k_compact2 is built from the generator's NaN flags
    ga.stage = generate_stage_bytes(r.kind, s.Bl) ? b.gen_stage : nullptr;
    // compaction / gather / fp16 operands of the hypotheses, built in the same launch as the hypothesis-ordered copies
    CompactArgs &ca = a.comp;
    ca.num_models = b.num_models;
    ca.B = s.Bl;
    ca.maxm = (int32_t)s.slots;
    ca.blk_tot = blk_tot;
    ca.slots = b.slots;
    ca.offsets = b.offsets;
    ca.models = b.models;
    ca.shadow = b.shadow;
    ca.compact64 = b.compact64;
    ca.ctl = b.ctl;
    if (live_list) { // absolute pose: the operand rows of the live hypotheses and of the correspondences
        ca.s16.out = b.shadow16;
        ca.s16.g16 = r.pf.g16, ca.s16.c16 = r.pf.c16, ca.s16.thr = r.pf.thr;
        ca.s16.live = b.live, ca.s16.rank = b.rank, ca.s16.nan_bits = ga.nan_bits;
        ca.s16.points16 = b.points16, ca.s16.point_rows = s.point_rows;
    } else if (s.use_mfma && r.kind == EST_HOM) { // homography: operands of k_score_mfmah (k_hom16)
        ca.s16.out = b.shadow16;
        ca.s16.sampson = 2;
        ca.s16.thr = r.pf.h16;
    } else if (s.use_mfma) { // two-view: operands of the Sampson forms (k_sampson16 / k_score_mfma2)
        ca.s16.out = b.shadow16;
        ca.s16.sampson = 1;
    }
    ca.host_offsets = nullptr; // (the one entry a stopping problem needs is fetched after the replay)
    // scorer
    ScoreArgs &sa = a.score;
    sa.pts = r.pts;
    sa.models = b.models;
    sa.slots = b.slots;
    sa.shadow = b.shadow;
    sa.compact64 = b.compact64;
    sa.shadow16 = ca.s16.out;
    sa.num_hyp = &b.ctl->num_hyp;
    if (live_list) { // the live list replaces the hypothesis list; everything else stays in the hypothesis index space
        sa.slots = b.live;
        sa.num_hyp = &b.ctl->num_live;
        sa.points16 = b.points16;
    }
    sa.hyp_capacity = (uint32_t)hcap;
    sa.thr2 = r.thr2;
    sa.pf = r.pf;
    sa.part_count = b.part_count;
    sa.part_score = b.part_score;
    sa.tickets = blk_tot + 2 * (size_t)nblk + 2;
    if (s.prune && live_list) { // lead, c*, selection (launch_score_pruned / launch_group_score)
        PruneArgs &pa = sa.prune;
        pa.st = reinterpret_cast<PruneState *>(b.prune_state);
        pa.blk_kept = reinterpret_cast<uint32_t *>(b.prune_state + kPruneTilesOffset);
        pa.sel = b.prune_sel;
        pa.kept = b.prune_kept;
        pa.chunks = s.chunks;
        pa.chunk_points = s.point_rows / s.chunks;
        pa.init_max = r.init_max, pa.init_min = r.init_min;
        pa.lead = kPruneLead;
        pa.bound = 1;
    }
    // finalize + records
    RecordsArgs &ra = a.rec;
    ra.f.num_hyp = &b.ctl->num_hyp;
    ra.f.rank = ca.s16.rank;
    ra.f.hyp_capacity = (uint32_t)hcap;
    ra.f.chunks = s.chunks;
    ra.f.n_points = r.pts.n;
    ra.f.thr2 = r.thr2;
    ra.f.part_count = b.part_count;
    ra.f.part_score = b.part_score;
    ra.f.count = b.count;
    ra.f.score = b.score;
    ra.f.kept = sa.prune.kept; // (nullptr: the step does not prune)
    ra.slots = b.slots;
    ra.models = b.models;
    ra.blk_max = reinterpret_cast<uint32_t *>(b.blk_best);
    ra.blk_min = reinterpret_cast<double *>(b.blk_best + kBlkMinOffset);
    ra.init_max = r.init_max;
    ra.init_min = r.init_min;
    ra.rec_meta = b.rec_meta;
    ra.rec_models = b.rec_models;
    ra.rec_cap = kRecordCap;
    ra.ctl = b.ctl;
    ra.host_meta = b.host_meta;
    ra.host_models = b.host_models;
    ra.host_cap = kRecordFirst;
    // the listed candidates once more, summed like the reference sums them (decisions are taken on these); this last kernel of
    // the step mirrors the control block into pinned host memory
    SeqScoreArgs &qa = a.seq;
    qa.pts = r.pts;
    qa.models = b.models;
    qa.cand = b.rec_meta;
    qa.num = &b.ctl->num_records;
    qa.cap = kRecordCap;
    qa.thr2 = r.thr2;
    qa.host_cand = b.host_meta;
    qa.host_cap = kRecordFirst;
    qa.ctl_src = b.ctl;
    qa.ctl_host = b.host_ctl;
}

// A member's part in the extents of a group's sampler launch (launch_group_positions: the grid of k_sample_delta_g, the build of
// k_sample_orbit_g); a fresh GroupDims starts with min_n = 0xffffffff.
void group_dims_sampler(GroupDims &d, uint32_t M, uint32_t n, uint32_t B) {
    d.max_M = std::max(d.max_M, M);
    d.min_n = std::min(d.min_n, n);
    d.max_B = std::max(d.max_B, B);
}

// The step's buffers in the Context (the single-problem path), grown to `z`.
int context_batch_buffers(Context *c, const BatchSizes &z, BatchBuffers &b) {
    auto grown = [](DevBuf &d, size_t bytes, auto *&ptr) {
        const hipError_t e = d.ensure(bytes);
        ptr = static_cast<std::remove_reference_t<decltype(ptr)>>(d.p);
        return e;
    };
    HIP_TRY(grown(c->positions, z.positions, b.positions));
    HIP_TRY(grown(c->delta, z.delta, b.delta));
    HIP_TRY(grown(c->flags, z.flags, b.flags));
    HIP_TRY(grown(c->samples, z.samples, b.samples));
    HIP_TRY(grown(c->models, z.models, b.models));
    HIP_TRY(grown(c->num_models, z.num_models, b.num_models));
    HIP_TRY(grown(c->nan_bits, z.nan_bits, b.nan_bits));
    HIP_TRY(grown(c->slots, z.slots, b.slots));
    HIP_TRY(grown(c->offsets, z.offsets, b.offsets));
    HIP_TRY(grown(c->ctl, z.ctl, b.ctl));
    HIP_TRY(grown(c->shadow, z.shadow, b.shadow));
    HIP_TRY(grown(c->compact64, z.compact64, b.compact64));
    HIP_TRY(grown(c->shadow16, z.shadow16, b.shadow16));
    HIP_TRY(grown(c->live, z.live, b.live));
    HIP_TRY(grown(c->rank, z.rank, b.rank));
    HIP_TRY(grown(c->points16, z.points16, b.points16));
    HIP_TRY(grown(c->part_count, z.part_count, b.part_count));
    HIP_TRY(grown(c->part_score, z.part_score, b.part_score));
    HIP_TRY(grown(c->count, z.count, b.count));
    HIP_TRY(grown(c->score, z.score, b.score));
    HIP_TRY(grown(c->blk_best, z.blk_best, b.blk_best));
    HIP_TRY(grown(c->rec_meta, z.rec_meta, b.rec_meta));
    HIP_TRY(grown(c->rec_models, z.rec_models, b.rec_models));
    HIP_TRY(grown(c->gen_stage, z.gen_stage, b.gen_stage));
    HIP_TRY(grown(c->prune_sel, z.prune_sel, b.prune_sel));
    HIP_TRY(grown(c->prune_kept, z.prune_kept, b.prune_kept));
    HIP_TRY(grown(c->prune_state, z.prune_state, b.prune_state));
    HIP_TRY(c->h_small.ensure(sizeof(BatchCtl) + 64));
    HIP_TRY(c->h_rec_meta.ensure(sizeof(RecordMeta) * kRecordCap));
    HIP_TRY(c->h_gather_out.ensure(sizeof(double) * kModelStride * kRecordCap));
    b.host_meta = c->h_rec_meta.dev<RecordMeta>();
    b.host_models = c->h_gather_out.dev<double>();
    b.host_ctl = c->h_small.dev<BatchCtl>();
    return PL_OK;
}

// Which kernel refines the camera-less jobs of one launch on a problem of `n` correspondences: 0 k_lm, 1 k_lm_ordered, 2 k_lm2 with
// `slices` workgroups per task.  run_refinements and the diagnostic pl_debug_lm_route both ask here.
// Large point sets with 6..8 parameters saturate the single CU k_lm gives a task; k_lm2 spreads every task over
// several workgroups (one launch per LM iteration; only for short, bounded runs - the LO: 25 iterations - since it
// costs max_iterations + 2 launches whatever the iteration count turns out to be).  Measured on MI355X at N = 10^4:
// homography problems 2.2x, fundamental 1.5x shorter when the device serves one problem at a time; with many
// problems in flight the long single-CU kernels overlap anyway and the extra launches cost throughput.  The two
// kernels sum the normal equations in different orders (results agree to rounding, not to the bit), so the choice
// must not depend on load or on the entry point: it is a process-wide setting, OFF by default - the grouped launches
// of pl_estimate_batch refine with k_lm, and a problem gives the same bits whichever way it is submitted -,
// POSELIB_AMD_LATENCY_MODE=1 switches it on for single large two-view problems.
struct LMRoute {
    int kernel;
    uint32_t slices;
};
LMRoute lm_route(int kind, uint32_t n, bool same_it, uint32_t max_it) {
    static const bool latency_mode = [] {
        const char *e = std::getenv("POSELIB_AMD_LATENCY_MODE");
        return e && e[0] == '1';
    }();
    const bool ordered = lm_sums_ordered(kind);
    const uint32_t lm2_min_points = (kind == EST_ABS) ? 8192u : 2560u;
    if (latency_mode && kind != EST_REL && kind != EST_RELT && kind != EST_RAD1D && !ordered && same_it && max_it >= 1 && max_it <= 32 && n >= lm2_min_points)
        return {2, std::min<uint32_t>(16u, std::max<uint32_t>(2u, n / 512u))};
    return {ordered ? 1 : 0, 0u};
}

struct RefineJob {
    double record_in[kModelStride]; // seed model
    LMOptions opt;
    CameraParams cam;
    double point_scale = 1.0;
    double prefilter_thr2 = 0.0;
    const uint8_t *d_mask = nullptr;
    int cam_flags = 0; // absolute pose: CamRefineFlags, the intrinsics refined with the pose (k_lm_cam)
    // outputs
    CameraParams cam_out;
    double record_out[kModelStride];
    double params_out[kParamDoubles];
    uint32_t count = 0;
    double score = 0;
    bool skipped = false;
};

// Optional tail of a single-job refinement: pick "refined if its score beats the incumbent's, else the incumbent"
// on the device (ransac_impl.h:190-198) and compute that model's inlier mask, all behind the same synchronisation.
struct MaskTail {
    double incumbent_score;      // stats.model_score
    const double *incumbent_rec; // host record of the incumbent (best model so far)
    double thr2;
    uint8_t *host_mask;          // N bytes or nullptr
    const MaskDest *dst = nullptr; // the caller's device copy or nullptr
};

// Runs all jobs as one batched LM launch; the refined parameters become records ON THE DEVICE (k_task_records),
// which are (optionally) re-scored with threshold thr2, and (optionally, single job) followed by the mask tail.
// One stream synchronisation for the whole chain.
int run_refinements(Context *c, const pl_problem *p, std::vector<RefineJob> &jobs, bool rescore, double thr2,
                    const MaskTail *tail = nullptr) {
    const uint32_t nj = (uint32_t)jobs.size();
    if (nj == 0)
        return PL_OK;
    // one staging block in pinned, device-mapped host memory: [LMTask x nj][seed records x nj (+ the incumbent's record)].
    // k_lm fetches its task from there itself (one cooperative read over the bus) and writes the outputs back, so the
    // single-workgroup path needs no upload dispatch; the multi-launch k_lm2 path reads its tasks every launch and keeps
    // a device copy.
    static_assert(sizeof(LMTask) % sizeof(double) == 0, "records follow the tasks");
    const size_t stage_bytes = sizeof(LMTask) * nj + sizeof(double) * kModelStride * (nj + 1);
    HIP_TRY(c->h_tasks.ensure(stage_bytes));
    HIP_TRY(c->lm_scratch.ensure((size_t)p->n * nj + 16));
    HIP_TRY(c->lm_records.ensure(sizeof(double) * kModelStride * nj));
    uint32_t max_it = 0;
    bool same_it = true;
    for (uint32_t j = 0; j < nj; ++j) {
        same_it = same_it && (j == 0 || jobs[j].opt.max_iterations == max_it);
        max_it = std::max(max_it, jobs[j].opt.max_iterations);
    }
    bool with_camera = false;
    for (uint32_t j = 0; j < nj; ++j)
        with_camera = with_camera || jobs[j].cam_flags != 0;
    if (with_camera && p->kind != EST_ABS)
        return fail(PL_ERR_INVALID, "camera intrinsics are refined with absolute poses only");
    const LMRoute route = lm_route(p->kind, p->n, same_it, max_it);
    const bool use_lm2 = !with_camera && route.kernel == 2;
    if (use_lm2)
        HIP_TRY(c->lm_tasks.ensure(stage_bytes));
    LMTask *ht = c->h_tasks.as<LMTask>();
    double *hr = reinterpret_cast<double *>(ht + nj);
    // where the kernels see the staging block: the device copy (k_lm2) or the pinned block itself (k_lm)
    LMTask *d_tasks = use_lm2 ? c->lm_tasks.as<LMTask>() : c->h_tasks.dev<LMTask>();
    double *d_records_in = reinterpret_cast<double *>(d_tasks + nj);
    for (uint32_t j = 0; j < nj; ++j) {
        LMTask &t = ht[j];
        std::memset(&t, 0, sizeof(t));
        t.pts = p->ps;
        lm_params_from_record(p->kind, jobs[j].record_in, t.params);
        t.opt = jobs[j].opt;
        t.cam = jobs[j].cam;
        t.point_scale = jobs[j].point_scale;
        t.cam_flags = jobs[j].cam_flags;
        t.prefilter_thr2 = jobs[j].prefilter_thr2;
        t.mask = jobs[j].d_mask;
        t.scratch = c->lm_scratch.as<uint8_t>() + (size_t)j * p->n;
        t.record_in = d_records_in + (size_t)j * kModelStride;
        t.record_out = use_lm2 ? nullptr : c->lm_records.as<double>() + (size_t)j * kModelStride;
        std::memcpy(hr + (size_t)j * kModelStride, jobs[j].record_in, sizeof(double) * kModelStride);
    }
    if (tail)
        std::memcpy(hr + (size_t)nj * kModelStride, tail->incumbent_rec, sizeof(double) * kModelStride);
    if (use_lm2) {
        HIP_TRY(hipMemcpyAsync(c->lm_tasks.p, ht, stage_bytes, hipMemcpyHostToDevice, c->stream));
        const uint32_t slices = route.slices;
        HIP_TRY(c->lm2_states.ensure(lm2_state_bytes(nj)));
        HIP_TRY(c->lm2_partials.ensure(lm2_partial_bytes(nj, slices)));
        bool loss_changes = false; // between the iterations of a task: it then takes up to two launches per iteration
        for (uint32_t j = 0; j < nj; ++j)
            loss_changes = loss_changes || jobs[j].opt.loss_type == LOSS_TRUNCATED_LE_ZACH;
        HIP_TRY(launch_lm2(p->kind, p->ps, d_tasks, nj, slices, max_it, loss_changes, c->lm2_states.p,
                           c->lm2_partials.as<double>(), c->stream));
        // (k_task_records also writes the tasks' outputs into the pinned staging block: stream order puts that after the
        // upload above has read it)
        HIP_TRY(launch_task_records(p->kind, d_tasks, d_records_in, c->lm_records.as<double>(), nj,
                                    c->h_tasks.dev<LMTask>(), c->stream));
    } else if (with_camera) { // (tasks of such a call without flags: M = 0 is not a k_lm_cam case)
        for (uint32_t j = 0; j < nj; ++j)
            if (!jobs[j].cam_flags)
                return fail(PL_ERR_INVALID, "refinement jobs with and without intrinsics in one launch");
        HIP_TRY(launch_lm_cam(d_tasks, nj, c->stream));
    } else {
        HIP_TRY(launch_lm(p->kind, p->ps, d_tasks, nj, c->stream)); // outputs + refined records: written by k_lm itself
    }
    if (rescore || tail) {
        int rc = enqueue_score_records(c, p, c->lm_records.as<double>(), nj, tail ? tail->thr2 : thr2);
        if (rc != PL_OK)
            return rc;
    }
    if (tail) { // single job: choose refined / incumbent on the device, then the inlier mask of the choice
        HIP_TRY(c->mask.ensure(std::max<uint32_t>(p->n, 1u)));
        HIP_TRY(c->tmp_model.ensure(sizeof(double) * kModelStride));
        HIP_TRY(launch_select_record(c->score.as<double>(), tail->incumbent_score, c->lm_records.as<double>(),
                                     d_records_in + (size_t)nj * kModelStride,
                                     c->tmp_model.as<double>(), c->stream));
        HIP_TRY(c->h_mask.ensure(std::max<uint32_t>(p->n, 1u)));
        HIP_TRY(launch_mask(p->kind, p->ps, c->tmp_model.as<double>(), tail->thr2, c->mask.as<uint8_t>(),
                            tail->host_mask ? c->h_mask.dev<uint8_t>() : nullptr, c->stream, tail->dst));
    }
    HIP_TRY(wait_stream(c));
    if (tail && tail->host_mask && p->n) // the kernel wrote the pinned copy itself
        std::memcpy(tail->host_mask, c->h_mask.p, p->n);
    for (uint32_t j = 0; j < nj; ++j) {
        jobs[j].skipped = ht[j].skipped != 0;
        std::memcpy(jobs[j].params_out, ht[j].params, sizeof(double) * kParamDoubles);
        jobs[j].cam_out = ht[j].cam;
        if (jobs[j].skipped) // refinement not run: model unchanged (relative_pose.cc:75-77)
            std::memcpy(jobs[j].record_out, jobs[j].record_in, sizeof(double) * kModelStride);
        else
            record_from_lm_params(p->kind, ht[j].params, jobs[j].record_out); // same inline function as the device
        if (rescore || tail) {
            jobs[j].count = c->h_count.as<uint32_t>()[j];
            jobs[j].score = c->h_score.as<double>()[j];
        }
    }
    return PL_OK;
}

struct Improving { // a minimal hypothesis that improved best_minimal_* (candidate for best_model)
    uint32_t iter;   // absolute iteration index
    uint32_t slot;   // model record index inside the batch
    uint32_t count;
    double score;
    bool lo_seed;    // last improving hypothesis of its iteration
    uint32_t gather; // index into the gathered record array
    int job = -1;    // index of the refinement job when lo_seed
};

// One LO-RANSAC run (ransac_impl.h:157-201) as batches: `enqueue_batch` puts the whole device pipeline of a batch of
// iterations on the stream, `collect_improving` synchronises once and lists the hypotheses that improved the running
// best, `exchange_improving` (sharded runs only) merges the ranks' lists, `refine_and_replay` runs the triggered local
// optimisations as one batched launch and replays the sequential loop over the batch, event by event.
struct RansacRun {
    static constexpr int kRedoBatch = 1; // positive: not an error, the batch has to be evaluated again

    // what one batch hands from step to step
    struct Batch {
        uint32_t B = 0;                      // iterations of the batch (all ranks)
        uint32_t lo_g = 0, hi_g = 0, Bl = 0; // this rank's share: iterations [it + lo_g, it + hi_g)
        size_t hcap = 0;                     // hypothesis capacity of the share
        BatchCtl *d_ctl = nullptr;
        uint64_t pos_after = 0; // sampler draws consumed after the batch
        bool device_positions = false;
        ProsacSampler prosac_at_batch_start; // a repeated batch draws the same samples
        bool overflow = false;               // an iteration of the share produced more models than slots
        uint32_t H = 0, H_local = 0;         // hypotheses of the batch (sharded: over all ranks) / of the share
        uint64_t b0_inl = 0;                 // state of the sequential loop at the start of the batch
        double b0_score = 0;
        const double *h_rec = nullptr; // model records of `imps`, indexed by Improving::gather
        bool ctl_mirrored = false;     // k_score_seq has written the control block to pinned host memory
    };

    Context *c;
    const pl_problem *p;
    const pl_robust_options *o;
    double *best_record; // in/out
    uint8_t *inliers;
    pl_ransac_stats *st;
    const int kind;
    const uint32_t N;
    const int K;
    int MAXM; // record slots per iteration (5-pt: grown to 40 on demand)
    const pl_ransac_options &ro;
    const double thr2;
    const LMOptions lo_opt;
    CameraParams null_cam;
    // one problem across several devices (pl_ransac_run_sharded): this rank evaluates a contiguous share of every batch
    const pl_shard *sh;
    const uint32_t G, grank;
    struct WireHead {
        uint32_t n, gen_overflow, H, pad;
    };
    struct WireRec {
        uint32_t iter_off, count; // iteration relative to the batch start
        double score;
        double model[kModelStride];
    };
    static constexpr uint32_t kWireFirst = 32; // records that travel with the header
    std::vector<unsigned char> wire_send, wire_recv;
    std::vector<double> merged_models;
    // state of the sequential loop
    uint64_t best_min_inl = 0;
    double best_min_score = std::numeric_limits<double>::max();
    uint64_t dyn_max;
    const double log_fail;
    uint64_t it = 0;  // next iteration to evaluate == iterations replayed so far
    uint64_t pos = 0; // sampler draws consumed so far
    bool stopped = false;
    std::vector<Improving> imps;
    std::vector<RefineJob> jobs;
    std::vector<uint32_t> order;
    // diagnostics: POSELIB_AMD_HOST_BOOKKEEPING=1 (both), POSELIB_AMD_HOST_POSITIONS=1 (sampler positions walked on the
    // host), POSELIB_AMD_HOST_RECORDS=1 (improving hypotheses found by a host scan over all scores)
    const bool host_bookkeeping = std::getenv("POSELIB_AMD_HOST_BOOKKEEPING") != nullptr;
    const bool host_positions = host_bookkeeping || std::getenv("POSELIB_AMD_HOST_POSITIONS") != nullptr;
    const bool host_records = host_bookkeeping || std::getenv("POSELIB_AMD_HOST_RECORDS") != nullptr;
    bool force_host_positions = false;
    const bool prosac;
    ProsacSampler prosac_sampler;

    RansacRun(Context *c_, const pl_problem *p_, const pl_robust_options *o_, double *best_record_, uint8_t *inliers_,
              pl_ransac_stats *st_)
        : c(c_), p(p_), o(o_), best_record(best_record_), inliers(inliers_), st(st_), kind(p_->kind), N(p_->n),
          K(sample_size(p_->kind)), MAXM((p_->kind == EST_REL || p_->kind == EST_RELT) ? 8 : max_models(p_->kind)), ro(o_->ransac),
          thr2(o_->max_error * o_->max_error), lo_opt(lo_options(o_->max_error)),
          sh((g_shard && g_shard->world > 1) ? g_shard : nullptr), G(sh ? (uint32_t)sh->world : 1u),
          grank(sh ? (uint32_t)sh->rank : 0u), dyn_max(o_->ransac.max_iterations),
          log_fail(std::log(1.0 - o_->ransac.success_prob)), prosac(o_->ransac.progressive_sampling != 0) {
        std::memset(&null_cam, 0, sizeof(null_cam));
        null_cam.model_id = CAM_NULL;
    }

    RefineJob make_lo_job(const double *rec) const {
        RefineJob j;
        std::memcpy(j.record_in, rec, sizeof(j.record_in));
        j.opt = lo_opt;
        j.cam = null_cam;
        j.point_scale = 1.0;
        j.prefilter_thr2 = (kind == EST_REL) ? 5 * thr2 : 0.0; // relative_pose.cc:70
        return j;
    }
    // A homography is a matrix up to scale AND sign, and two local optimisations that started from minimal models of opposite
    // sign end in the same optimum as H and -H with scores that agree to the last few bits: which of them `score < best` keeps
    // hangs on the bits of the refined models, i.e. on the order the normal equations are summed in.  Beyond 256 correspondences
    // the default sums run in tree order (models 1e-13 off the reference's), and in one of ~1000 default-option problems the
    // caller got -H (tests/parity_soak_estimate_batch.py 4000 11, item 1186; every other field identical).  A local
    // optimisation is a function of its seed - the minimal model, whose bits ARE the reference's - so when such a decision
    // comes up (opposite signs, scores within 2e-15: the tree order moves a converged model's score by an ulp or two) the two
    // refinements are repeated with the sums in the reference's order (k_lm_ordered) and the decision is taken on those
    // results, which are the reference's bit for bit.  Up to 4096 correspondences: there the ordered kernel costs 1.3 - 2 x the
    // tree kernel for the one or two tasks concerned (< 0.5 % of the default-option homography problems; with a bound of 1e-13,
    // 1.5 % of them, the synchronous launches inside the groups' replays cost a 512-problem batch call 17 %); at 10^4 it costs 6 x
    // and long runs meet such a pair about once each - that regime keeps the tree order (pl_set_lm_mode(1) pins it).
    double best_seed[kModelStride];                  // the minimal model the incumbent was refined from ...
    bool best_from_lo = false, best_exact = false;   // ... if it is a refined one / already refined in the reference's order
    static constexpr double kSignTieGap = 2e-15; // (9 ulps of the score: the tree order moves a converged model's score by an ulp or two)
    static constexpr uint32_t kSignTieMaxPoints = 4096;
    int resolve_sign_tie(RefineJob &job) {
        // (a sharded run: every rank holds the whole problem and replays the same decisions - each repeats the two refinements itself)
        if (kind != EST_HOM || N <= (uint32_t)kLMSeqPoints || N > kSignTieMaxPoints || lm_sums_ordered(EST_HOM) || job.skipped ||
            !(st->model_score < std::numeric_limits<double>::max()) ||
            !(std::fabs(job.score - st->model_score) <= kSignTieGap * std::fabs(st->model_score)))
            return PL_OK;
        double dot = 0;
        for (int i = 0; i < 9; ++i)
            dot += job.record_out[kMatOff + i] * best_record[kMatOff + i];
        if (!(dot < 0))
            return PL_OK;
        std::vector<RefineJob> exact{make_lo_job(job.record_in)};
        const bool both = best_from_lo && !best_exact;
        if (both)
            exact.push_back(make_lo_job(best_seed));
        set_lm_force_ordered(1);
        const int rc = run_refinements(c, p, exact, true, thr2);
        set_lm_force_ordered(0);
        if (rc != PL_OK)
            return rc;
        job.score = exact[0].score, job.count = exact[0].count, job.skipped = exact[0].skipped;
        std::memcpy(job.record_out, exact[0].record_out, sizeof(job.record_out));
        std::memcpy(job.params_out, exact[0].params_out, sizeof(job.params_out));
        if (both) {
            st->model_score = exact[1].score;
            st->num_inliers = exact[1].count;
            std::memcpy(best_record, exact[1].record_out, sizeof(double) * kModelStride);
            best_exact = true;
        }
        job_exact = true;
        return PL_OK;
    }
    bool job_exact = false;
    int after_lo(RefineJob &job) { // ransac_impl.h:138-153
        st->refinements++;
        job_exact = false;
        const int rc_tie = resolve_sign_tie(job);
        if (rc_tie != PL_OK)
            return rc_tie;
        if (job.score < st->model_score) {
            st->model_score = job.score;
            st->num_inliers = job.count;
            std::memcpy(best_record, job.record_out, sizeof(double) * kModelStride);
            std::memcpy(best_seed, job.record_in, sizeof(best_seed));
            best_from_lo = true;
            best_exact = job_exact;
        }
        st->inlier_ratio = static_cast<double>(st->num_inliers) / static_cast<double>(N);
        dyn_max = dynamic_max_iter(st->num_inliers, N, K, log_fail, ro.dyn_num_trials_mult, ro.min_iterations,
                                   ro.max_iterations);
        return PL_OK;
    }

    int score_initial_model() {
        HIP_TRY(c->tmp_model.ensure(sizeof(double) * kModelStride));
        HIP_TRY(hipMemcpyAsync(c->tmp_model.p, best_record, sizeof(double) * kModelStride, hipMemcpyHostToDevice,
                               c->stream));
        int rc = enqueue_score_records(c, p, c->tmp_model.as<double>(), 1, thr2);
        if (rc != PL_OK)
            return rc;
        HIP_TRY(wait_stream(c));
        const uint32_t cnt = c->h_count.as<uint32_t>()[0];
        const double sc = c->h_score.as<double>()[0];
        const bool more = cnt > best_min_inl, better = sc < best_min_score;
        if (more || better) {
            if (more)
                best_min_inl = cnt;
            if (better)
                best_min_score = sc;
            if (sc < st->model_score) {
                st->model_score = sc;
                st->num_inliers = cnt;
            }
            std::vector<RefineJob> jobs{make_lo_job(best_record)};
            rc = run_refinements(c, p, jobs, true, thr2);
            if (rc != PL_OK)
                return rc;
            rc = after_lo(jobs[0]);
            if (rc != PL_OK)
                return rc;
        }
        return PL_OK;
    }

    // the state the next batch step starts from
    BatchRun batch_run() const {
        BatchRun r;
        r.kind = kind;
        r.pts = p->ps;
        r.seed = ro.seed;
        r.pos = pos;
        r.thr2 = thr2;
        r.pf = problem_prefilter(p, thr2);
        r.init_max = (uint32_t)std::min<uint64_t>(best_min_inl, 0xffffffffu);
        r.init_min = best_min_score;
        r.real_focal_check = o->real_focal_check;
        r.explicit_samples = prosac;
        return r;
    }

    // ---- device: positions -> generate -> compact -> score -> finalize -> records, all on the stream ----
    int enqueue_batch(Batch &b) {
        const BatchRun run = batch_run();
        BatchShape s;
        s.B = b.B, s.lo = b.lo_g, s.Bl = b.Bl, s.M = 0, s.slots = (uint32_t)MAXM;
        s.use_mfma = score_uses_mfma(kind, N, run.pf);
        s.chunks = score_chunks(kind, N, true, s.use_mfma);
        s.point_rows = abs16_point_rows(N);
        // (no pruning here, whatever score_prune_gate says of the step: this launch is ONE resident round of workgroups, chunks that
        // return at once leave their compute units idle and the lead, the selection and the second scorer launch come on top -
        // measured with the one-tier form: 0.113 -> 0.269 ms per step of the flagship problem, profiles/score_prune.md; the two-tier
        // form was not measured on this path.  The single launches of the pruned form stay behind
        // pl_debug_score_pruned route 0.)
        s.prune = false;
        b.device_positions = !host_positions && !force_host_positions && !prosac;
        if (b.device_positions) {
            const uint64_t M64 = sampler_window(N, K, s.B); // window of draw positions to evaluate
            if (M64 > 0x7fffffffull || pos + M64 >= 0xffffffffull)
                b.device_positions = false;
            else
                s.M = (uint32_t)M64;
        }
        const BatchSizes z = batch_step_sizes(kind, s);
        BatchBuffers bb;
        const int rc = context_batch_buffers(c, z, bb);
        if (rc != PL_OK)
            return rc;
        GroupArgs a;
        wire_batch_step(a, run, s, bb);
        b.hcap = a.score.hyp_capacity;
        b.d_ctl = bb.ctl;
        b.prosac_at_batch_start = prosac_sampler; // a repeated batch draws the same samples

        if (prosac) {
            HIP_TRY(c->h_positions.ensure(z.samples));
            uint32_t *hs = c->h_positions.as<uint32_t>();
            for (uint32_t i = 0; i < s.B; ++i)
                prosac_sampler.generate(hs + (size_t)i * K);
            b.pos_after = prosac_sampler.pos;
            if (s.Bl)
                HIP_TRY(hipMemcpyAsync(bb.samples, hs + (size_t)s.lo * K, sizeof(uint32_t) * (size_t)s.Bl * K,
                                       hipMemcpyHostToDevice, c->stream));
        }
        if (b.device_positions) // (its first kernel clears the control block; otherwise a memset does)
            HIP_TRY(launch_sample_positions(K, a.samp, c->stream));
        else
            HIP_TRY(hipMemsetAsync(bb.ctl, 0, z.ctl, c->stream));
        if (!b.device_positions && !prosac) {
            HIP_TRY(c->h_positions.ensure(z.positions));
            b.pos_after = sample_positions_k(K, ro.seed, pos, N, s.B, c->h_positions.as<uint32_t>());
            if (b.pos_after - pos >= 0xffffffffull)
                return fail(PL_ERR_UNSUPPORTED, "sampler draw window exceeds 32 bits");
            HIP_TRY(hipMemcpyAsync(bb.positions, c->h_positions.p, z.positions, hipMemcpyHostToDevice, c->stream));
        }
        if (s.Bl > 0) { // (a rank whose share of a short batch is empty only takes part in the exchange)
            const uint32_t slices = std::max<uint32_t>(1u, std::min<uint32_t>(1536u / s.chunks, a.score.hyp_capacity));
            HIP_TRY(launch_generate(kind, a.gen, c->stream));
            HIP_TRY(launch_compact2(a.comp, true, p->ps, c->stream));
            HIP_TRY(hipEventRecord(c->ev0, c->stream));
            if (a.score.prune.st)
                HIP_TRY(launch_score_pruned(a.score, slices, c->stream));
            else
                HIP_TRY(launch_score(kind, a.score, slices, c->stream));
            HIP_TRY(hipEventRecord(c->ev1, c->stream));
            HIP_TRY(launch_finalize_records(a.rec, c->stream));
            HIP_TRY(launch_score_seq(kind, a.seq, c->stream));
            b.ctl_mirrored = true;
        }
        return PL_OK;
    }

    // The n candidates of one batch (scores summed in the reference's order), sorted by hypothesis index, through the rule of
    // ransac_impl.h:113-123: those that improve the running best become `imps`; the last one of an iteration seeds
    // the local optimisation.  first_iteration: absolute index of the first iteration of the batch (of this rank's share).
    void list_improving(const RecordMeta *meta, uint32_t n, uint32_t first_iteration) {
        imps.clear();
        order.resize(n);
        for (uint32_t a = 0; a < n; ++a)
            order[a] = a;
        std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return meta[x].k < meta[y].k; });
        for (uint32_t a = 0; a < n; ++a) {
            const RecordMeta &m = meta[order[a]];
            const bool more = m.count > best_min_inl, better = m.score < best_min_score;
            if (!(more || better))
                continue;
            if (more)
                best_min_inl = m.count;
            if (better)
                best_min_score = m.score;
            Improving im;
            im.iter = first_iteration + m.slot / (uint32_t)MAXM;
            im.slot = m.slot;
            im.count = m.count;
            im.score = m.score;
            im.lo_seed = false;
            im.gather = order[a];
            if (!imps.empty() && imps.back().iter != im.iter)
                imps.back().lo_seed = true;
            imps.push_back(im);
        }
        if (!imps.empty())
            imps.back().lo_seed = true;
    }

    // ---- the one synchronisation of the batch; retry decisions; improving hypotheses of this rank's share ----
    int collect_improving(Batch &b) {
        const uint32_t B = b.B, lo_g = b.lo_g, Bl = b.Bl;
        const size_t hcap = b.hcap;
        BatchCtl *const d_ctl = b.d_ctl;
        uint64_t &pos_after = b.pos_after;
        const bool device_positions = b.device_positions;
        const ProsacSampler &prosac_at_batch_start = b.prosac_at_batch_start;
        BatchCtl *h_ctl = c->h_small.as<BatchCtl>();
        RecordMeta *h_meta = c->h_rec_meta.as<RecordMeta>(); // the first kRecordFirst candidates: written by k_score_seq
        double *h_recm = c->h_gather_out.as<double>();
        if (!b.ctl_mirrored)
            HIP_TRY(hipMemcpyAsync(h_ctl, d_ctl, sizeof(BatchCtl), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(wait_stream(c));
        if (device_positions) {
            if (h_ctl->orbit_error) { // evaluated window too small / too many redraws: redo this batch
                force_host_positions = true;
                return kRedoBatch;
            }
            pos_after = h_ctl->pos_after;
            static const bool check_positions = std::getenv("POSELIB_AMD_CHECK_POSITIONS") != nullptr;
            if (check_positions) { // diagnostic: the device's orbit walk against the sequential walk on the host
                std::vector<uint32_t> dev(B), host(B);
                HIP_TRY(hipMemcpy(dev.data(), c->positions.p, sizeof(uint32_t) * B, hipMemcpyDeviceToHost));
                const uint64_t after = sample_positions_k(K, ro.seed, pos, N, B, host.data());
                for (uint32_t i = 0; i < B; ++i)
                    if (dev[i] != host[i]) {
                        std::fprintf(stderr, "poselib_amd: sampler position mismatch: N %u K %d batch %u at draw %llu, iteration %u: device %u host %u\n",
                                     N, K, B, (unsigned long long)pos, i, dev[i], host[i]);
                        return fail(PL_ERR_HIP, "device sampler positions differ from the sequential walk");
                    }
                if (after != pos_after) {
                    std::fprintf(stderr, "poselib_amd: sampler end position mismatch: device %llu host %llu\n",
                                 (unsigned long long)pos_after, (unsigned long long)after);
                    return fail(PL_ERR_HIP, "device sampler end position differs from the sequential walk");
                }
            }
        }
        const bool overflow = h_ctl->gen_overflow != 0;
        if (overflow && !sh) { // an iteration produced more models than the reserved slots: redo with 40
            MAXM = max_models(kind);
            prosac_sampler = prosac_at_batch_start;
            return kRedoBatch;
        } // (sharded: the ranks agree on the retry in the exchange below)
        force_host_positions = false;
        uint32_t H = h_ctl->num_hyp; // sharded: replaced by the sum over the ranks after the exchange
        const uint32_t H_local = H;
        if (Bl > 0 && !overflow) {
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
            st->score_kernel_ms += ms;
            st->score_kernel_launches++;
            st->nan_hypotheses += h_ctl->nan_hyp;
        }
        const uint64_t b0_inl = best_min_inl; // state of the sequential loop at the start of the batch
        const double b0_score = best_min_score;

        // ---- pass 1 result: the improving hypotheses, in (iteration, model) order ----
        imps.clear();
        const double *h_rec = h_recm;
        const uint32_t nrec = overflow ? 0u : h_ctl->num_records;
        if (overflow) {
            // nothing to report: every rank redoes the batch with more slots per iteration
        } else if (!host_records && nrec <= kRecordCap) {
            if (nrec > kRecordFirst) {
                HIP_TRY(hipMemcpyAsync(h_meta, c->rec_meta.p, sizeof(RecordMeta) * nrec, hipMemcpyDeviceToHost,
                                       c->stream));
                HIP_TRY(hipMemcpyAsync(h_recm, c->rec_models.p, sizeof(double) * kModelStride * nrec,
                                       hipMemcpyDeviceToHost, c->stream));
                HIP_TRY(wait_stream(c));
            }
            list_improving(h_meta, nrec, (uint32_t)(it + lo_g));
        } else {
            // fallback (candidate list overflow, or POSELIB_AMD_HOST_RECORDS=1): scan every (tree-order) score on the
            // host with the same margin as k_records, have the candidates re-scored in the reference's summation
            // order, then apply the exact rule like above
            HIP_TRY(c->h_num_models.ensure(sizeof(uint32_t) * (Bl + 1)));
            HIP_TRY(c->h_count.ensure(sizeof(uint32_t) * hcap));
            HIP_TRY(c->h_score.ensure(sizeof(double) * hcap));
            uint32_t *h_nm = c->h_num_models.as<uint32_t>();
            if (Bl)
                HIP_TRY(hipMemcpyAsync(h_nm, c->num_models.p, sizeof(uint32_t) * Bl, hipMemcpyDeviceToHost, c->stream));
            if (H) {
                HIP_TRY(hipMemcpyAsync(c->h_count.p, c->count.p, sizeof(uint32_t) * H, hipMemcpyDeviceToHost,
                                       c->stream));
                HIP_TRY(hipMemcpyAsync(c->h_score.p, c->score.p, sizeof(double) * H, hipMemcpyDeviceToHost,
                                       c->stream));
            }
            HIP_TRY(wait_stream(c));
            const uint32_t *h_cnt = c->h_count.as<uint32_t>();
            const double *h_sc = c->h_score.as<double>();
            std::vector<RecordMeta> cand;
            uint64_t run_inl = best_min_inl;
            double run_score = best_min_score;
            uint32_t k = 0;
            for (uint32_t i = 0; i < Bl; ++i)
                for (uint32_t m = 0; m < h_nm[i]; ++m, ++k) {
                    if (!(h_cnt[k] > run_inl || h_sc[k] < run_score * (1.0 + 1e-9)))
                        continue;
                    run_inl = std::max<uint64_t>(run_inl, h_cnt[k]);
                    run_score = std::min(run_score, h_sc[k]);
                    RecordMeta rm;
                    rm.k = k;
                    rm.slot = i * MAXM + m;
                    rm.count = h_cnt[k];
                    rm.pad = 0;
                    rm.score = h_sc[k];
                    cand.push_back(rm);
                }
            const uint32_t nc = (uint32_t)cand.size();
            HIP_TRY(c->h_rec_meta.ensure(sizeof(RecordMeta) * std::max<uint32_t>(nc, kRecordCap)));
            HIP_TRY(c->h_gather_out.ensure(sizeof(double) * kModelStride * std::max<uint32_t>(nc, kRecordCap)));
            h_meta = c->h_rec_meta.as<RecordMeta>();
            double *dst = c->h_gather_out.as<double>();
            if (nc) {
                HIP_TRY(c->rec_meta.ensure(sizeof(RecordMeta) * std::max<uint32_t>(nc, kRecordCap)));
                HIP_TRY(c->num_hyp.ensure(sizeof(uint32_t)));
                std::memcpy(h_meta, cand.data(), sizeof(RecordMeta) * nc);
                HIP_TRY(hipMemcpyAsync(c->rec_meta.p, h_meta, sizeof(RecordMeta) * nc, hipMemcpyHostToDevice, c->stream));
                HIP_TRY(hipMemcpyAsync(c->num_hyp.p, &nc, sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
                SeqScoreArgs qa;
                qa.pts = p->ps;
                qa.models = c->models.as<double>();
                qa.cand = c->rec_meta.as<RecordMeta>();
                qa.num = c->num_hyp.as<uint32_t>();
                qa.cap = nc;
                qa.thr2 = thr2;
                qa.count = nullptr;
                qa.score = nullptr;
                qa.host_count = nullptr;
                qa.host_score = nullptr;
                qa.host_cand = nullptr;
                qa.host_cap = 0;
                HIP_TRY(launch_score_seq(kind, qa, c->stream));
                HIP_TRY(hipMemcpyAsync(h_meta, c->rec_meta.p, sizeof(RecordMeta) * nc, hipMemcpyDeviceToHost, c->stream));
                for (uint32_t a = 0; a < nc; ++a)
                    HIP_TRY(hipMemcpyAsync(dst + (size_t)a * kModelStride,
                                           c->models.as<double>() + (size_t)cand[a].slot * kModelStride,
                                           sizeof(double) * kModelStride, hipMemcpyDeviceToHost, c->stream));
                HIP_TRY(wait_stream(c));
            }
            list_improving(h_meta, nc, (uint32_t)(it + lo_g)); // (the scan listed them by hypothesis index already)
            h_rec = dst;
        }

        b.overflow = overflow;
        b.H = H;
        b.H_local = H_local;
        b.b0_inl = b0_inl;
        b.b0_score = b0_score;
        b.h_rec = h_rec;
        return PL_OK;
    }

    // ---- sharded runs: first exchange step of the batch (all-gather of the ranks' improving hypotheses) ----
    int exchange_improving(Batch &b) {
        const bool overflow = b.overflow;
        const uint32_t H_local = b.H_local;
        const uint64_t b0_inl = b.b0_inl;
        const double b0_score = b.b0_score;
        const ProsacSampler &prosac_at_batch_start = b.prosac_at_batch_start;
        uint32_t &H = b.H;
        const double *&h_rec = b.h_rec;
        // ---- sharded: the first exchange step of the batch.  Every rank contributes the improving hypotheses of its
        // range (improving w.r.t. the batch-start state and its own earlier hypotheses - a superset of what the
        // sequential loop keeps); the merged list is filtered with the true running best, rank by rank, i.e. in
        // iteration order.  From here on every rank holds the same list and does the same thing. ----
        if (sh) {
            const uint32_t nloc = (uint32_t)imps.size();
            auto pack = [&](unsigned char *dst, uint32_t first, uint32_t count) {
                for (uint32_t a = 0; a < count; ++a) {
                    WireRec w;
                    std::memset(&w, 0, sizeof(w));
                    if (first + a < nloc) {
                        const Improving &im = imps[first + a];
                        w.iter_off = (uint32_t)(im.iter - it);
                        w.count = im.count;
                        w.score = im.score;
                        std::memcpy(w.model, h_rec + (size_t)im.gather * kModelStride, sizeof(w.model));
                    }
                    std::memcpy(dst + (size_t)a * sizeof(WireRec), &w, sizeof(w));
                }
            };
            const size_t bytes1 = sizeof(WireHead) + (size_t)kWireFirst * sizeof(WireRec);
            wire_send.assign(bytes1, 0);
            wire_recv.assign(bytes1 * G, 0);
            WireHead head{nloc, overflow ? 1u : 0u, H_local, 0u};
            std::memcpy(wire_send.data(), &head, sizeof(head));
            pack(wire_send.data() + sizeof(WireHead), 0, kWireFirst);
            if (sh->allgather(sh->user, wire_send.data(), wire_recv.data(), bytes1) != 0)
                return fail(PL_ERR_COMM, "all-gather callback failed");
            std::vector<WireHead> heads(G);
            bool any_overflow = false;
            uint32_t max_n = 0;
            uint64_t H_sum = 0;
            for (uint32_t r = 0; r < G; ++r) {
                std::memcpy(&heads[r], wire_recv.data() + (size_t)r * bytes1, sizeof(WireHead));
                any_overflow = any_overflow || heads[r].gen_overflow != 0;
                max_n = std::max(max_n, heads[r].n);
                H_sum += heads[r].H;
            }
            if (any_overflow) { // some rank ran out of model slots: all ranks redo the batch with 40 per iteration
                best_min_inl = b0_inl;
                best_min_score = b0_score;
                MAXM = max_models(kind);
                prosac_sampler = prosac_at_batch_start;
                return kRedoBatch;
            }
            const unsigned char *recs = wire_recv.data() + sizeof(WireHead);
            size_t rank_stride = bytes1;
            std::vector<unsigned char> recv2;
            if (max_n > kWireFirst) { // rare: a second message with every rank's full list
                const size_t bytes2 = (size_t)max_n * sizeof(WireRec);
                std::vector<unsigned char> send2(bytes2, 0);
                recv2.assign(bytes2 * G, 0);
                pack(send2.data(), 0, max_n);
                if (sh->allgather(sh->user, send2.data(), recv2.data(), bytes2) != 0)
                    return fail(PL_ERR_COMM, "all-gather callback failed");
                recs = recv2.data();
                rank_stride = bytes2;
            }
            imps.clear();
            merged_models.clear();
            uint64_t run_inl = b0_inl;
            double run_score = b0_score;
            for (uint32_t r = 0; r < G; ++r)
                for (uint32_t a = 0; a < heads[r].n; ++a) {
                    WireRec w;
                    std::memcpy(&w, recs + (size_t)r * rank_stride + (size_t)a * sizeof(WireRec), sizeof(w));
                    const bool more = w.count > run_inl, better = w.score < run_score; // ransac_impl.h:114-116
                    if (!(more || better))
                        continue;
                    if (more)
                        run_inl = w.count;
                    if (better)
                        run_score = w.score;
                    Improving im;
                    im.iter = (uint32_t)(it + w.iter_off);
                    im.slot = 0;
                    im.count = w.count;
                    im.score = w.score;
                    im.lo_seed = false;
                    im.gather = (uint32_t)imps.size();
                    if (!imps.empty() && imps.back().iter != im.iter)
                        imps.back().lo_seed = true;
                    imps.push_back(im);
                    merged_models.insert(merged_models.end(), w.model, w.model + kModelStride);
                }
            if (!imps.empty())
                imps.back().lo_seed = true;
            best_min_inl = run_inl;
            best_min_score = run_score;
            h_rec = merged_models.data();
            H = (uint32_t)std::min<uint64_t>(H_sum, 0xffffffffu);
        }
        return PL_OK;
    }

    // Sharded runs: the local optimisations of a batch are dealt out to the ranks (job j to rank j mod world; the
    // kernels are deterministic, so it does not matter which device refines a seed) and their results - refined record,
    // inlier count, score - are all-gathered: the second (and last) exchange step of a batch, ~0.2 KB per job.
    int run_refinements_sharded() {
        struct WireJob {
            double record_out[kModelStride];
            double score;
            uint32_t count, skipped;
        };
        const uint32_t nj = (uint32_t)jobs.size();
        const uint32_t per_rank = (nj + G - 1) / G;
        std::vector<RefineJob> mine;
        for (uint32_t j = grank; j < nj; j += G)
            mine.push_back(jobs[j]);
        if (!mine.empty()) {
            const int rc = run_refinements(c, p, mine, true, thr2);
            if (rc != PL_OK)
                return rc;
        }
        const size_t bytes = (size_t)per_rank * sizeof(WireJob);
        wire_send.assign(bytes, 0);
        wire_recv.assign(bytes * G, 0);
        for (uint32_t a = 0; a < (uint32_t)mine.size(); ++a) {
            WireJob w;
            std::memset(&w, 0, sizeof(w));
            std::memcpy(w.record_out, mine[a].record_out, sizeof(w.record_out));
            w.score = mine[a].score;
            w.count = mine[a].count;
            w.skipped = mine[a].skipped ? 1u : 0u;
            std::memcpy(wire_send.data() + (size_t)a * sizeof(WireJob), &w, sizeof(w));
        }
        if (sh->allgather(sh->user, wire_send.data(), wire_recv.data(), bytes) != 0)
            return fail(PL_ERR_COMM, "all-gather callback failed");
        for (uint32_t j = 0; j < nj; ++j) {
            WireJob w;
            std::memcpy(&w, wire_recv.data() + (size_t)(j % G) * bytes + (size_t)(j / G) * sizeof(WireJob), sizeof(w));
            std::memcpy(jobs[j].record_out, w.record_out, sizeof(w.record_out));
            jobs[j].score = w.score;
            jobs[j].count = w.count;
            jobs[j].skipped = w.skipped != 0;
        }
        return PL_OK;
    }

    // ---- the local optimisations the batch's improving hypotheses trigger (ransac_impl.h:127-131: the last improving
    // hypothesis of an iteration seeds one) ----
    void make_jobs(const Batch &b) {
        const uint32_t ni = (uint32_t)imps.size();
        jobs.clear();
        for (uint32_t a = 0; a < ni; ++a)
            if (imps[a].lo_seed) {
                imps[a].job = (int)jobs.size();
                jobs.push_back(make_lo_job(b.h_rec + (size_t)imps[a].gather * kModelStride));
            }
    }

    // ---- batched local optimisations of the batch, then the replay of the sequential loop over it ----
    int refine_and_replay(Batch &b) {
        // ---- device: every triggered LO of the batch as one batched launch, then re-scored ----
        make_jobs(b);
        if (!jobs.empty()) {
            const int rc = sh ? run_refinements_sharded() : run_refinements(c, p, jobs, true, thr2);
            if (rc != PL_OK)
                return rc;
        }
        return replay(b, nullptr);
    }

    // ---- host pass 2: replay the sequential loop over this batch (ransac_impl.h:180-188) with the refined and
    // re-scored models in `jobs`.  host_offsets: pinned mirror of the per-iteration hypothesis offsets of the batch (group
    // launches write one); nullptr: the one entry that is needed is fetched from the device ----
    // (defer_offset: group launches - the caller fetches offsets[deferred_offset] of all stopping problems in one go and
    // books it into st->hypotheses; mirroring the whole table to pinned memory cost 0.4 MB of PCIe writes per problem and batch)
    bool defer_offset = false;
    int64_t deferred_offset = -1;
    int replay(Batch &b, const uint32_t *host_offsets) {
        const uint32_t B = b.B, lo_g = b.lo_g, hi_g = b.hi_g, Bl = b.Bl;
        (void)B, (void)lo_g, (void)hi_g, (void)Bl;
        const uint32_t H = b.H, H_local = b.H_local;
        const double *const h_rec = b.h_rec;
        const uint64_t pos_after = b.pos_after;
        st->iterations_evaluated += B;
        const uint32_t ni = (uint32_t)imps.size();

        // The stop rule can only change at LO events, so the replay hops from event to event.
        uint64_t cursor = it;          // next iteration whose stop check has not been made yet
        uint64_t stop_at = it + B;     // first iteration NOT replayed
        for (uint32_t a = 0; a < ni; ++a) {
            const Improving &im = imps[a];
            const uint64_t first_stop = std::max<uint64_t>(std::max<uint64_t>(ro.min_iterations, dyn_max) + 1, cursor);
            if (first_stop <= im.iter) {
                stopped = true;
                stop_at = first_stop;
                break;
            }
            if (im.score < st->model_score) { // :126-131
                st->model_score = im.score;
                st->num_inliers = im.count;
                std::memcpy(best_record, h_rec + (size_t)im.gather * kModelStride, sizeof(double) * kModelStride);
                best_from_lo = false; // (a minimal model: its bits are the reference's)
            }
            if (im.lo_seed) {
                const int rc_lo = after_lo(jobs[im.job]);
                if (rc_lo != PL_OK)
                    return rc_lo;
            }
            cursor = (uint64_t)im.iter + 1;
        }
        if (!stopped) {
            const uint64_t first_stop = std::max<uint64_t>(std::max<uint64_t>(ro.min_iterations, dyn_max) + 1, cursor);
            if (first_stop < it + B) {
                stopped = true;
                stop_at = first_stop;
            }
        }
        if (stop_at < it + B) { // hypotheses of the replayed iterations only
            uint32_t upto = 0;
            if (stop_at >= it + hi_g) {
                upto = H_local;
            } else if (stop_at > it + lo_g) {
                if (host_offsets) {
                    upto = host_offsets[stop_at - it - lo_g];
                } else if (defer_offset && !sh) {
                    deferred_offset = (int64_t)(stop_at - it - lo_g);
                } else {
                    HIP_TRY(hipMemcpyAsync(&upto, c->offsets.as<uint32_t>() + (stop_at - it - lo_g), sizeof(uint32_t),
                                           hipMemcpyDeviceToHost, c->stream));
                    HIP_TRY(wait_stream(c));
                }
            }
            uint64_t total = upto;
            if (sh) { // sum of the ranks' shares (8 bytes each; once per run)
                std::vector<uint64_t> all(G, 0);
                if (sh->allgather(sh->user, &total, all.data(), sizeof(uint64_t)) != 0)
                    return fail(PL_ERR_COMM, "all-gather callback failed");
                total = 0;
                for (uint32_t r = 0; r < G; ++r)
                    total += all[r];
            }
            st->hypotheses += total;
        } else {
            st->hypotheses += H;
        }
        it = stop_at;
        pos = pos_after;
        return PL_OK;
    }

    // ---- size of the next batch (false: the loop is over) ----
    uint64_t grow = 0;
    void begin_loop() {
        // batch capacity: bounded by the scratch the model records need
        grow = std::max<uint64_t>(ro.min_iterations + 2, 512);
        grow = (grow + 63) / 64 * 64;
        if (prosac)
            prosac_sampler.init(ro.seed, N, K, ro.max_prosac_iterations);
    }
    // iterations the loop is known to need at least from here (plan_batch's bound, without its side effects)
    uint64_t needed_now() const {
        uint64_t needed = std::max<uint64_t>(ro.min_iterations, dyn_max) + 1;
        needed = std::min<uint64_t>(needed, ro.max_iterations);
        return (needed > it) ? needed - it : 1;
    }
    bool plan_batch(Batch &b) {
        if (stopped || it >= ro.max_iterations)
            return false;
        if (it > ro.min_iterations && it > dyn_max) { // stop rule at the top of the next iteration (:182)
            stopped = true;
            return false;
        }
        // the loop cannot stop before max(min_iterations, dynamic_max_iter) + 1 iterations
        uint64_t needed = std::max<uint64_t>(ro.min_iterations, dyn_max) + 1;
        needed = std::min<uint64_t>(needed, ro.max_iterations);
        needed = (needed > it) ? needed - it : 1;
        const uint32_t cap = std::min<uint32_t>(131072u, 1048576u / (uint32_t)MAXM); // scratch size (<= 200 MB of records)
        b = Batch();
        b.B = (uint32_t)std::min<uint64_t>({needed, (uint64_t)cap, grow, ro.max_iterations - it});
        grow = std::min<uint64_t>(grow * 2, 131072u);
        // this rank's share of the batch (the whole batch on a single device)
        b.lo_g = (uint32_t)((uint64_t)b.B * grank / G);
        b.hi_g = (uint32_t)((uint64_t)b.B * (grank + 1) / G);
        b.Bl = b.hi_g - b.lo_g;
        return true;
    }

    int run() {
        std::memset(st, 0, sizeof(*st));
        st->model_score = std::numeric_limits<double>::max();
        const double t_start = now_s();
        bool mask_done = false;
        if (N >= (uint32_t)K) { // ransac_impl.h:161-163
            st->num_inliers = 0;
            if (ro.score_initial_model) {
                const int rc = score_initial_model();
                if (rc != PL_OK)
                    return rc;
            }
            begin_loop();
            Batch b;
            while (plan_batch(b)) {
                int rc = enqueue_batch(b);
                if (rc == PL_OK)
                    rc = collect_improving(b);
                if (rc == PL_OK && sh)
                    rc = exchange_improving(b);
                if (rc == kRedoBatch)
                    continue;
                if (rc == PL_OK)
                    rc = refine_and_replay(b);
                if (rc != PL_OK)
                    return rc;
            }
            st->iterations = it;

            // ---- final refinement of the best model (ransac_impl.h:190-198; model_score is not updated), chained on the
            // device with the choice refined / incumbent and the inlier mask of the returned model (ransac.cc:55, 152,
            // 259, 311): one synchronisation ----
            {
                std::vector<RefineJob> fin{make_lo_job(best_record)};
                MaskTail tail;
                tail.incumbent_score = st->model_score;
                tail.incumbent_rec = best_record;
                tail.thr2 = thr2;
                tail.host_mask = inliers;
                tail.dst = g_mask_dest;
                int rc = run_refinements(c, p, fin, true, thr2, &tail);
                if (rc != PL_OK)
                    return rc;
                st->refinements++;
                if (fin[0].score < st->model_score) {
                    std::memcpy(best_record, fin[0].record_out, sizeof(double) * kModelStride);
                    st->num_inliers = fin[0].count;
                }
                mask_done = true;
            }
        }

        // ---- inlier mask of the returned model when the loop did not run (too few points: ransac_impl.h:161-163) ----
        if (N > 0 && !mask_done) {
            HIP_TRY(c->mask.ensure(N));
            HIP_TRY(c->tmp_model.ensure(sizeof(double) * kModelStride));
            HIP_TRY(hipMemcpyAsync(c->tmp_model.p, best_record, sizeof(double) * kModelStride, hipMemcpyHostToDevice,
                                   c->stream));
            HIP_TRY(c->h_mask.ensure(N));
            HIP_TRY(launch_mask(kind, p->ps, c->tmp_model.as<double>(), thr2, c->mask.as<uint8_t>(),
                                inliers ? c->h_mask.dev<uint8_t>() : nullptr, c->stream, g_mask_dest));
            HIP_TRY(wait_stream(c));
            if (inliers)
                std::memcpy(inliers, c->h_mask.p, N);
        }
        st->seconds = now_s() - t_start;
        return PL_OK;
    }
};

int ransac_core(Context *c, const pl_problem *p, const pl_robust_options *o, double *best_record /* in/out */,
                uint8_t *inliers, pl_ransac_stats *st) {
    RansacRun run(c, p, o, best_record, inliers, st);
    return run.run();
}

int validate_options(const pl_robust_options *o, bool focal_entry = false) {
    if (!o)
        return fail(PL_ERR_INVALID, "options pointer is null");
    if (o->min_fov != o->min_fov) // (a record shorter than this library's - built against an older header - reads garbage here)
        return fail(PL_ERR_INVALID, "min_fov is NaN (options record not filled by pl_default_robust_options, or built against another PL_ABI_VERSION?)");
    // estimate_focal_length: pl_estimate_absolute_pose only (robust.cc:47-54 -> ransac_pnpf, driver_focal.inc)
    if (focal_entry && o->estimate_focal_length && !o->tangent_sampson && !o->estimate_extra_params)
        return PL_OK;
    // (bundle.refine_*: used by the absolute-pose front-end's final bundle, robust.cc:103-123; the other front-ends'
    // refiners have no camera to move, the reference ignores the flags there and so does this library)
    if (o->tangent_sampson || o->estimate_focal_length || o->estimate_extra_params)
        return fail(PL_ERR_UNSUPPORTED, "tangent-Sampson errors, estimate_extra_params and - outside pl_estimate_absolute_pose - "
                                        "estimate_focal_length are outside the accelerated hot path");
    return PL_OK;
}

// scale_a: factor of the first point set on its way into the SoA block (1D-radial front-end, robust.cc:904-907; x * 1.0 = x elsewhere)
int make_problem(Context *c, int kind, const double *a, const double *b, size_t n, pl_problem *p, double scale_a = 1.0) {
    if ((kind < 0 || kind > 3) && kind != EST_RAD1D)
        return fail(PL_ERR_INVALID, "unknown problem kind");
    if (n > 0x7fffffffu)
        return fail(PL_ERR_INVALID, "too many correspondences");
    p->kind = kind;
    p->device = c->device;
    p->n = (uint32_t)n;
    p->d_pts = nullptr;
    const int nd = point_doubles(kind);
    const int da = 2, db = (kind == EST_ABS || kind == EST_RAD1D) ? 3 : 2;
    std::memset(&p->ps, 0, sizeof(p->ps));
    p->ps.n = (uint32_t)n;
    if (n == 0)
        return PL_OK;
    std::vector<double> soa((size_t)nd * n);
    double amax = 0;
    for (size_t i = 0; i < n; ++i) {
        for (int d = 0; d < da; ++d) {
            soa[(size_t)d * n + i] = a[da * i + d] * scale_a;
            const double v = std::fabs(soa[(size_t)d * n + i]);
            amax = (v > amax || v != v) ? v : amax; // NaN propagates and disables the pre-filter
        }
        for (int d = 0; d < db; ++d) {
            soa[(size_t)(da + d) * n + i] = b[db * i + d];
            if (kind != EST_ABS && kind != EST_RAD1D) { // two-view: the bound covers all four coordinates (pl_prefilter.h, fp16 Sampson form)
                const double v = std::fabs(b[db * i + d]);
                amax = (v > amax || v != v) ? v : amax;
            }
        }
    }
    HIP_TRY(hipMalloc((void **)&p->d_pts, sizeof(double) * nd * n));
    hipError_t up = hipMemcpyAsync(p->d_pts, soa.data(), sizeof(double) * nd * n, hipMemcpyHostToDevice, c->stream);
    if (up == hipSuccess)
        up = hipStreamSynchronize(c->stream);
    if (up != hipSuccess) {
        (void)hipFree(p->d_pts);
        p->d_pts = nullptr;
        return fail(PL_ERR_HIP, "upload of the correspondences", up);
    }
    for (int d = 0; d < nd; ++d)
        p->ps.a[d] = p->d_pts + (size_t)d * n;
    p->ps.xy_absmax = std::nextafter((float)amax, std::numeric_limits<float>::infinity());
    return PL_OK;
}
void free_problem(pl_problem *p) {
    if (p->d_pts && !p->borrowed)
        (void)hipFree(p->d_pts);
    p->d_pts = nullptr;
}

// The bound of max(|x|, |y|) of the prepared points that keeps the scorers' fp32 / fp16 pre-filters conservative (pl_prefilter.h).
// Absolute pose through a linear camera and two-view problems from 1024 correspondences on (the matrix-core Sampson form; the O(N)
// host pass is not worth it below) get it from the raw points on the host; absolute pose through a non-linear camera (OPENCV,
// SIMPLE_RADIAL, RADIAL, the fisheye models: camera_is_nonlinear) reads k_prepare's atomic max back (the un-projection is iterative); smaller two-view problems get none (+inf).  make_problem_prepared and the groups'
// stage A both decide it here.

// upper bound of max(|x|, |y|) of the un-projected 2-D points of a linear camera (the un-projected coordinate is (px - c) / f up to
// one rounding)
float host_xy_absmax(const CameraParams &cam, const double *a, size_t n) {
    double cx = 0, cy = 0, fx = 1, fy = 1;
    if (cam.model_id == CAM_SIMPLE_PINHOLE)
        fx = fy = cam.p[0], cx = cam.p[1], cy = cam.p[2];
    else if (cam.model_id == CAM_PINHOLE)
        fx = cam.p[0], fy = cam.p[1], cx = cam.p[2], cy = cam.p[3];
    double m = 0.0;
    for (size_t i = 0; i < n; ++i) {
        const double u = std::fabs((a[2 * i] - cx) / fx), v = std::fabs((a[2 * i + 1] - cy) / fy);
        m = (u > m || u != u) ? u : m; // NaN propagates (and disables the pre-filter)
        m = (v > m || v != v) ? v : m;
    }
    m = m * (1.0 + 1e-12);
    return std::nextafter((float)m, std::numeric_limits<float>::infinity());
}
// Upper bound of the largest |coordinate| the prepared two-view points will have (pl_prefilter.h, fp16 Sampson form), from
// the raw points on the host: linear cameras / the normalisation (x - c) / scale round at most once per operation.
// +inf when it cannot be told without the device (a non-linear camera's un-projection) or a coordinate is NaN.
float host_two_view_absmax(const PrepareArgs &pa, const double *a, const double *b, size_t n) {
    const float inf = std::numeric_limits<float>::infinity();
    double m = 0.0;
    auto take = [&](double v) { m = (v > m || v != v) ? v : m; };
    if (pa.mode == 1) {
        const CameraParams *cams[2] = {&pa.cam1, &pa.cam2};
        const double *pts[2] = {a, b};
        for (int k = 0; k < 2; ++k) {
            const CameraParams &cam = *cams[k];
            double cx = 0, cy = 0, fx = 1, fy = 1;
            if (cam.model_id == CAM_SIMPLE_PINHOLE)
                fx = fy = cam.p[0], cx = cam.p[1], cy = cam.p[2];
            else if (cam.model_id == CAM_PINHOLE)
                fx = cam.p[0], fy = cam.p[1], cx = cam.p[2], cy = cam.p[3];
            else if (cam.model_id != CAM_NULL)
                return inf;
            for (size_t i = 0; i < n; ++i) {
                take(std::fabs((pts[k][2 * i] - cx) / fx));
                take(std::fabs((pts[k][2 * i + 1] - cy) / fy));
            }
        }
    } else if (pa.mode == 2) {
        const double c1x = pa.centred ? pa.c1x : 0.0, c1y = pa.centred ? pa.c1y : 0.0;
        const double c2x = pa.centred ? pa.c2x : 0.0, c2y = pa.centred ? pa.c2y : 0.0;
        for (size_t i = 0; i < n; ++i) {
            take(std::fabs((a[2 * i] - c1x) / pa.scale));
            take(std::fabs((a[2 * i + 1] - c1y) / pa.scale));
            take(std::fabs((b[2 * i] - c2x) / pa.scale));
            take(std::fabs((b[2 * i + 1] - c2y) / pa.scale));
        }
    } else {
        return inf;
    }
    if (m != m)
        return inf;
    m = m * (1.0 + 1e-12);
    return std::nextafter((float)m, inf);
}
bool prefilter_bound_on_device(int kind, const PrepareArgs &pa) {
    return kind == EST_ABS && !(pa.mode == 0 && !camera_is_nonlinear(pa.cam1.model_id));
}
// the bound when it comes from the host (prefilter_bound_on_device false)
float host_prefilter_bound(int kind, const PrepareArgs &pa, const double *a, const double *b, size_t n) {
    if (kind == EST_ABS)
        return host_xy_absmax(pa.cam1, a, n);
    if (n >= 1024 && a && b)
        return host_two_view_absmax(pa, a, b, n);
    return std::numeric_limits<float>::infinity();
}

// One-shot front-ends: the user's AoS buffers go to the device as they are and k_prepare (pipeline.hip) writes the SoA
// block into the context's arena - per-point un-projection / normalisation on the GPU, no
// hipMalloc / hipFree per call.  The problem is valid until the next make_problem_prepared on this thread.
// resident: the raw correspondences of this call are already in c->raw_a / raw_b (second preparation of the same
// inputs: no upload); lm_only: the problem is only refined on, never scored - no max|x| read-back, no synchronisation
// bound: the pre-filter bound when the caller already has it (the *_dev front-ends: a and b are then not read); otherwise the host pass
int make_problem_prepared(Context *c, int kind, const double *a, const double *b, size_t n, const PrepareArgs &pa,
                          pl_problem *p, bool resident = false, bool lm_only = false, const float *bound = nullptr) {
    if (kind < 0 || kind > EST_RELT)
        return fail(PL_ERR_INVALID, "unknown problem kind");
    if (n > 0x7fffffffu / (kind == EST_RELT ? 18u : 1u))
        return fail(PL_ERR_INVALID, "too many correspondences");
    p->kind = kind;
    p->device = c->device;
    p->n = (uint32_t)n;
    p->d_pts = nullptr;
    p->borrowed = true;
    std::memset(&p->ps, 0, sizeof(p->ps));
    p->ps.n = (uint32_t)n;
    if (n == 0)
        return PL_OK;
    const int nd = point_doubles(kind);
    const int db = (kind == EST_ABS) ? 3 : 2;
    HIP_TRY(c->pts_arena.ensure(sizeof(double) * nd * n));
    HIP_TRY(c->absmax.ensure(sizeof(unsigned long long)));
    HIP_TRY(c->h_absmax.ensure(sizeof(unsigned long long)));
    // max|x| of the prepared points is read back only for absolute-pose problems of non-linear cameras (prefilter_bound_on_device): no
    // fill dispatch in front of the others (k_prepare's atomic max then lands on a word nobody reads)
    const bool reads_absmax = !lm_only && prefilter_bound_on_device(kind, pa);
    if (reads_absmax)
        HIP_TRY(hipMemsetAsync(c->absmax.p, 0, sizeof(unsigned long long), c->stream));
    if (!resident) {
        const size_t bytes_a = sizeof(double) * 2 * n, bytes_b = sizeof(double) * db * n;
        if (bytes_a + bytes_b <= ((size_t)8 << 20)) {
            // through a pinned, mapped block k_prepare reads directly: no copy dispatches, and no copy from pageable memory (which pins
            // and unpins the caller's buffer under the process's memory-map lock - what front-end calls from many host threads
            // queued on, DESIGN 4 "focal estimators")
            HIP_TRY(c->h_in.ensure(bytes_a + bytes_b));
            std::memcpy(c->h_in.p, a, bytes_a);
            std::memcpy(c->h_in.as<char>() + bytes_a, b, bytes_b);
            c->raw_src_a = c->h_in.dev<double>();
            c->raw_src_b = reinterpret_cast<const double *>(c->h_in.dev<char>() + bytes_a);
        } else {
            HIP_TRY(c->raw_a.ensure(bytes_a));
            HIP_TRY(c->raw_b.ensure(bytes_b));
            HIP_TRY(hipMemcpyAsync(c->raw_a.p, a, bytes_a, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(hipMemcpyAsync(c->raw_b.p, b, bytes_b, hipMemcpyHostToDevice, c->stream));
            c->raw_src_a = c->raw_a.as<double>();
            c->raw_src_b = c->raw_b.as<double>();
        }
    }
    if (!c->raw_src_a || !c->raw_src_b)
        return fail(PL_ERR_INVALID, "second preparation without a first");
    HIP_TRY(launch_prepare(c->raw_src_a, c->raw_src_b, (uint32_t)n, pa, c->pts_arena.as<double>(),
                           c->absmax.as<unsigned long long>(), c->stream));
    p->d_pts = c->pts_arena.as<double>();
    if (kind == EST_RELT) { // one block of 18 arrays behind a[0] (pl_kernels.h); its pre-filter takes no bound of the coordinates
        p->ps.a[0] = p->d_pts;
        p->ps.xy_absmax = std::numeric_limits<float>::infinity();
        return PL_OK;
    }
    for (int d = 0; d < nd; ++d)
        p->ps.a[d] = p->d_pts + (size_t)d * n;
    if (!reads_absmax) { // (stream order puts the next kernels behind k_prepare)
        p->ps.xy_absmax = lm_only ? std::numeric_limits<float>::infinity() : bound ? *bound : host_prefilter_bound(kind, pa, a, b, n);
        return PL_OK;
    }
    HIP_TRY(hipMemcpyAsync(c->h_absmax.p, c->absmax.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(wait_stream(c));
    double amax;
    std::memcpy(&amax, c->h_absmax.p, sizeof(double));
    p->ps.xy_absmax = std::nextafter((float)amax, std::numeric_limits<float>::infinity());
    return PL_OK;
}
PrepareArgs prepare_unproject(const CameraParams &c1, const CameraParams *c2) {
    PrepareArgs pa;
    std::memset(&pa, 0, sizeof(pa));
    pa.mode = c2 ? 1 : 0;
    pa.cam1 = c1;
    if (c2)
        pa.cam2 = *c2;
    pa.scale = 1.0;
    return pa;
}

// user model <-> record
void record_from_pose(const pl_camera_pose *pose, bool essential, double *rec) {
    Quat q;
    q.w = pose->q[0], q.x = pose->q[1], q.y = pose->q[2], q.z = pose->q[3];
    store_pose_model_q(rec, q, v3(pose->t[0], pose->t[1], pose->t[2]), essential);
}
void pose_from_record(const double *rec, pl_camera_pose *pose) {
    for (int i = 0; i < 4; ++i)
        pose->q[i] = rec[i];
    for (int i = 0; i < 3; ++i)
        pose->t[i] = rec[4 + i];
}
Mat3 mat_from_colmajor(const double *m) {
    Mat3 A;
    for (int j = 0; j < 3; ++j)
        for (int i = 0; i < 3; ++i)
            A.m[3 * i + j] = m[3 * j + i];
    return A;
}
void mat_to_colmajor(const Mat3 &A, double *m) {
    for (int j = 0; j < 3; ++j)
        for (int i = 0; i < 3; ++i)
            m[3 * j + i] = A.m[3 * i + j];
}
Mat3 transpose3(const Mat3 &A) {
    Mat3 T;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            T.m[3 * i + j] = A.m[3 * j + i];
    return T;
}
void normalize_frobenius(Mat3 &A) {
    double s = 0;
    for (int j = 0; j < 3; ++j)
        for (int i = 0; i < 3; ++i)
            s += A.m[3 * i + j] * A.m[3 * i + j];
    const double n = std::sqrt(s);
    for (int i = 0; i < 9; ++i)
        A.m[i] /= n;
}

// the caller's model (pl_camera_pose for absolute / relative pose, column-major 3 x 3 for F / H) <-> record
void record_from_model(int kind, const void *model, double *rec) {
    if (kind == EST_ABS || kind == EST_REL || kind == EST_RELT || kind == EST_RAD1D)
        record_from_pose(static_cast<const pl_camera_pose *>(model), kind == EST_REL || kind == EST_RELT, rec);
    else
        store_matrix_model(rec, mat_from_colmajor(static_cast<const double *>(model)));
}
void model_from_record(int kind, const double *rec, void *model) {
    if (kind == EST_ABS || kind == EST_REL || kind == EST_RELT || kind == EST_RAD1D) {
        pose_from_record(rec, static_cast<pl_camera_pose *>(model));
    } else {
        Mat3 M;
        for (int i = 0; i < 9; ++i)
            M.m[i] = rec[kMatOff + i];
        mat_to_colmajor(M, static_cast<double *>(model));
    }
}

int run_with_model(Context *c, pl_problem *p, const pl_robust_options *o, void *model, uint8_t *inliers,
                   pl_ransac_stats *st) {
    double rec[kModelStride];
    if (o->ransac.score_initial_model && p->kind != EST_RELT) // (tangent Sampson: the identity whatever the caller's model, ransac.cc:159-160)
        record_from_model(p->kind, model, rec);
    else
        identity_record(p->kind, rec);
    int rc = ransac_core(c, p, o, rec, inliers, st);
    if (rc != PL_OK)
        return rc;
    model_from_record(p->kind, rec, model);
    return PL_OK;
}

// Final polish on the inliers (device mask from ransac_core is still in c->mask).
int final_refine(Context *c, pl_problem *p, const double *record_in, const LMOptions &opt, const CameraParams &cam,
                 double point_scale, double *record_out, double *params_out, int cam_flags = 0,
                 CameraParams *cam_out = nullptr) {
    RefineJob j;
    std::memcpy(j.record_in, record_in, sizeof(j.record_in));
    j.opt = opt;
    j.cam = cam;
    j.point_scale = point_scale;
    j.prefilter_thr2 = 0.0;
    j.d_mask = c->mask.as<uint8_t>();
    j.cam_flags = cam_flags;
    std::vector<RefineJob> jobs{j};
    int rc = run_refinements(c, p, jobs, false, 0.0);
    if (rc != PL_OK)
        return rc;
    if (cam_out)
        *cam_out = jobs[0].cam_out;
    std::memcpy(record_out, jobs[0].record_out, sizeof(double) * kModelStride);
    if (params_out)
        std::memcpy(params_out, jobs[0].params_out, sizeof(double) * kParamDoubles);
    return PL_OK;
}

// PoseLib/robust/utils.cc:584-644 with normalize_scale = shared_scale = true.  Only the two order-dependent reductions
// (centroids, mean distance) are summed here, sequentially like the reference; the per-point part - subtract the
// centroid, divide by the scale - is applied by k_prepare on the device with the same two operations per coordinate.
struct PointNorm { // the two reductions: centroids (zero when the points are not centred) and the mean distance / sqrt(2)
    double c1x = 0, c1y = 0, c2x = 0, c2y = 0, scale = 0;
};
PointNorm host_point_norm(const double *x1, const double *x2, size_t n, bool centroid) {
    PointNorm pn;
    double c1x = 0, c1y = 0, c2x = 0, c2y = 0;
    if (centroid) {
        for (size_t k = 0; k < n; ++k) {
            c1x += x1[2 * k], c1y += x1[2 * k + 1];
            c2x += x2[2 * k], c2y += x2[2 * k + 1];
        }
        c1x /= static_cast<double>(n), c1y /= static_cast<double>(n);
        c2x /= static_cast<double>(n), c2y /= static_cast<double>(n);
    }
    double scale = 0.0;
    for (size_t k = 0; k < n; ++k) {
        double a0 = x1[2 * k], a1 = x1[2 * k + 1], b0 = x2[2 * k], b1 = x2[2 * k + 1];
        if (centroid)
            a0 -= c1x, a1 -= c1y, b0 -= c2x, b1 -= c2y;
        scale += std::sqrt(a0 * a0 + a1 * a1);
        scale += std::sqrt(b0 * b0 + b1 * b1);
    }
    scale /= std::sqrt(2) * n;
    pn.c1x = c1x, pn.c1y = c1y, pn.c2x = c2x, pn.c2y = c2y, pn.scale = scale;
    return pn;
}
// the transforms and k_prepare's arguments from the reductions - summed on the host (above) or by k_point_stats (the *_dev front-ends)
double normalization_from(const PointNorm &pn, bool centroid, Mat3 &T1, Mat3 &T2, PrepareArgs &pa) {
    for (int i = 0; i < 9; ++i)
        T1.m[i] = T2.m[i] = (i % 4 == 0) ? 1.0 : 0.0;
    if (centroid) {
        T1.m[2] = -pn.c1x, T1.m[5] = -pn.c1y;
        T2.m[2] = -pn.c2x, T2.m[5] = -pn.c2y;
    }
    const double scale = pn.scale;
    const double f = 1.0 / scale;
    for (int i = 0; i < 6; ++i) {
        T1.m[i] *= f;
        T2.m[i] *= f;
    }
    std::memset(&pa, 0, sizeof(pa));
    pa.mode = 2;
    pa.centred = centroid ? 1 : 0;
    pa.c1x = pn.c1x, pa.c1y = pn.c1y, pa.c2x = pn.c2x, pa.c2y = pn.c2y;
    pa.scale = scale;
    return scale;
}
double normalization_of(const double *x1, const double *x2, size_t n, bool centroid, Mat3 &T1, Mat3 &T2,
                        PrepareArgs &pa) {
    return normalization_from(host_point_norm(x1, x2, n, centroid), centroid, T1, T2, pa);
}

// ---------------------------------------------------------------------------- front-ends (robust.cc)
// What a front-end of robust.cc does around its ransac_* call: the loop's options and point preparation, the warm start in the
// loop's coordinates, the inlier gate and set-up of the final bundle, the result in the caller's representation.  Written once,
// for the single-problem entry points (pl_estimate_*) and pl_estimate_batch's groups alike.
struct FrontEnd {
    int kind = 0;
    pl_robust_options scaled; // options of the ransac_* part (thresholds rescaled the way the front-end does)
    double scale = 1.0;       // abs: 1 / focal; rel: mean inverse focal; hom / fund: normalisation scale
    Mat3 T1, T2;              // hom / fund normalisation
    PrepareArgs prep{};       // un-projection / normalisation of the points (k_prepare)
    CameraParams cam{};       // abs: the caller's camera
    int cam_flags = 0;        // abs: CamRefineFlags of the final bundle (bundle.refine_*), 0 = pose alone
};

// abs: the final bundle's options - bundle.refine_focal_length forced when the focal length was estimated (robust.cc:53)
pl_bundle_options front_bundle_options(const pl_robust_options &opt) {
    pl_bundle_options bundle = opt.bundle;
    if (opt.estimate_focal_length)
        bundle.refine_focal_length = 1; // "force refinement of focal in this case"
    return bundle;
}

// homography / fundamental: are the points centred before they are scaled?  (robust.cc:552-562, 720-726)
bool front_centred(int kind, const pl_robust_options &opt) { return kind == EST_HOM || !opt.real_focal_check; }

// robust.cc:40-46 (abs), 249-253 / 286-292 (rel), 552-562 (fund), 720-726 (hom)
// norm: the reductions of the homography / fundamental normalisation (not read for the other kinds)
void front_begin_with(FrontEnd &fe, int kind, const PointNorm &norm, const pl_robust_options &opt, const pl_camera *camera1,
                      const pl_camera *camera2) {
    fe.kind = kind;
    fe.scaled = opt;
    std::memset(&fe.prep, 0, sizeof(fe.prep));
    std::memset(&fe.cam, 0, sizeof(fe.cam));
    fe.cam_flags = 0;
    switch (kind) {
    case EST_ABS:
        fe.cam = to_cam(camera1);
        fe.scale = 1.0 / camera_focal(camera1);
        fe.scaled.max_error *= fe.scale;
        fe.prep = prepare_unproject(fe.cam, nullptr);
        fe.cam_flags = active_cam_flags(fe.cam.model_id, front_bundle_options(opt));
        break;
    case EST_REL: {
        fe.scale = 0.5 * (1.0 / camera_focal(camera1) + 1.0 / camera_focal(camera2));
        fe.scaled.max_error *= fe.scale;
        fe.scaled.bundle.loss_scale *= fe.scale;
        const CameraParams c1 = to_cam(camera1), c2 = to_cam(camera2);
        fe.prep = prepare_unproject(c1, &c2);
        break;
    }
    case EST_RELT: { // robust.cc:249-265: pixels and cameras times the mean inverse focal length, then bearing + Jacobian per pixel
        fe.scale = 0.5 * (1.0 / camera_focal(camera1) + 1.0 / camera_focal(camera2));
        fe.scaled.max_error *= fe.scale;
        fe.scaled.bundle.loss_scale *= fe.scale;
        fe.scaled.tangent_sampson = 0; // (the kind carries it from here on)
        fe.prep.mode = 3;
        fe.prep.cam1 = to_cam(camera1), fe.prep.cam2 = to_cam(camera2);
        camera_rescale(fe.prep.cam1, fe.scale);
        camera_rescale(fe.prep.cam2, fe.scale);
        fe.prep.scale = fe.scale;
        break;
    }
    default:
        fe.scale = normalization_from(norm, front_centred(kind, opt), fe.T1, fe.T2, fe.prep);
        fe.scaled.max_error /= fe.scale;
        fe.scaled.bundle.loss_scale /= fe.scale;
        break;
    }
}
// ... with the reductions from the caller's host arrays
void front_begin(FrontEnd &fe, int kind, const double *a, const double *b, size_t n, const pl_robust_options &opt,
                 const pl_camera *camera1, const pl_camera *camera2) {
    PointNorm norm;
    if (kind == EST_FUND || kind == EST_HOM)
        norm = host_point_norm(a, b, n, front_centred(kind, opt));
    front_begin_with(fe, kind, norm, opt, camera1, camera2);
}

// the record the loop starts from: the identity, or with ransac.score_initial_model the caller's model - poses as they are, F and H
// in the normalised coordinates of the problem (robust.cc:566-569, 729-732)
void front_initial_record(const FrontEnd &fe, const void *model, double *rec) {
    // (tangent Sampson: ransac_relpose with cameras resets best_model unconditionally, ransac.cc:159-160 - with score_initial_model
    // the identity is what gets scored)
    if (!fe.scaled.ransac.score_initial_model || fe.kind == EST_RELT) {
        identity_record(fe.kind, rec);
        return;
    }
    if (fe.kind == EST_ABS || fe.kind == EST_REL) {
        record_from_model(fe.kind, model, rec);
        return;
    }
    Mat3 M = mat_from_colmajor(static_cast<const double *>(model));
    if (fe.kind == EST_FUND)
        M = mul(mul(inverse3(transpose3(fe.T2)), M), inverse3(fe.T1));
    else
        M = mul(mul(fe.T2, M), inverse3(fe.T1));
    normalize_frobenius(M);
    store_matrix_model(rec, M);
}

// the final bundle runs when the loop's model has MORE inliers than this (robust.cc:103, 296, 573, 736; shared focal :401)
constexpr int kFrontSharedFocal = 4; // (pl_batch_item.kind of the shared-focal relative pose)
uint64_t front_min_inliers(int kind) {
    switch (kind) {
    case EST_ABS:
        return 3;
    case EST_REL:
    case EST_RELT:
        return 5;
    case EST_FUND:
        return 7;
    case EST_HOM:
        return 4;
    default: // kFrontSharedFocal
        return 6;
    }
}

// the final bundle over the inliers (robust.cc:103-123: abs in focal-normalised pixels, bundle.refine_* intrinsics with the pose;
// 296-311, 573-588, 736-751: the others in the loop's coordinates)
struct FrontBundle {
    LMOptions opt;
    CameraParams cam;
    int cam_flags;
    double point_scale;
};
FrontBundle front_bundle(const FrontEnd &fe) {
    FrontBundle fb;
    std::memset(&fb.cam, 0, sizeof(fb.cam));
    if (fe.kind == EST_ABS) {
        pl_bundle_options b = front_bundle_options(fe.scaled);
        b.loss_scale = fe.scaled.bundle.loss_scale * fe.scale;
        fb.cam = fe.cam;
        camera_rescale(fb.cam, fe.scale);
        fb.opt = to_lm(b);
        fb.cam_flags = fe.cam_flags;
        fb.point_scale = fe.scale;
    } else {
        fb.opt = to_lm(fe.scaled.bundle);
        fb.cam.model_id = CAM_NULL;
        fb.cam_flags = 0;
        fb.point_scale = 1.0;
    }
    return fb;
}
// abs with the focal length estimated (robust.cc:52): the camera takes the loop's focal length, the bundle's scale follows it
void front_set_focal(FrontEnd &fe, pl_camera *camera, double focal) {
    camera_set_focal(camera, focal / fe.scale);
    fe.cam = to_cam(camera);
    fe.scale = 1.0 / camera_focal(camera);
}

// the result in the caller's representation.  abs: when the bundle ran (camera not null), the camera through the reference's
// camera.rescale(scale) ... rescale(1 / scale) round trip (robust.cc:119-121), with the intrinsics the bundle moved (cam_refined);
// fund / hom: back to pixels (robust.cc:590-591, 753-754)
void front_finish(const FrontEnd &fe, const double *rec, const CameraParams *cam_refined, void *model, pl_camera *camera) {
    if (fe.kind == EST_ABS || fe.kind == EST_REL || fe.kind == EST_RELT || fe.kind == EST_RAD1D) {
        model_from_record(fe.kind, rec, model);
        if (!camera)
            return;
        CameraParams back = fe.cam;
        camera_rescale(back, fe.scale);
        if (fe.cam_flags)
            back = *cam_refined;
        camera_rescale(back, 1.0 / fe.scale);
        for (int i = 0; i < camera->num_params && i < 12; ++i)
            camera->params[i] = back.p[i];
        return;
    }
    Mat3 M;
    for (int i = 0; i < 9; ++i)
        M.m[i] = rec[kMatOff + i];
    if (fe.kind == EST_FUND)
        M = mul(mul(transpose3(fe.T2), M), fe.T1);
    else
        M = mul(mul(inverse3(fe.T2), M), fe.T1);
    normalize_frobenius(M);
    mat_to_colmajor(M, static_cast<double *>(model));
}

// ---------------------------------------------------------------------------- the focal-length loops (pl_focal.h)
// the loop's options from the (rescaled) robust options; max_focal: absolute_pose.h:78 (-1: none)
FocalLoopOptions focal_loop_options(const pl_robust_options &o, double max_focal) {
    FocalLoopOptions lo;
    lo.max_iterations = o.ransac.max_iterations;
    lo.min_iterations = o.ransac.min_iterations;
    lo.seed = o.ransac.seed;
    lo.dyn_num_trials_mult = o.ransac.dyn_num_trials_mult;
    lo.success_prob = o.ransac.success_prob;
    lo.score_initial_model = o.ransac.score_initial_model != 0;
    lo.max_error = o.max_error;
    lo.progressive_sampling = o.ransac.progressive_sampling != 0; // sampling.cc:85-136, host-drawn (absolute_pose.h:80 / relative_pose.h:155: sampler(num_data, sample_sz, opt.ransac))
    lo.max_prosac_iterations = o.ransac.max_prosac_iterations;
    lo.max_focal = max_focal;
    return lo;
}
void stats_from_focal_loop(const FocalLoopStats &fs, pl_ransac_stats *st) {
    st->refinements = fs.refinements;
    st->iterations = fs.iterations;
    st->num_inliers = fs.num_inliers;
    st->inlier_ratio = fs.inlier_ratio;
    st->model_score = fs.model_score;
    st->hypotheses = fs.hypotheses;
    st->iterations_evaluated = fs.iterations_evaluated;
}
// compute_max_focal_length (absolute_pose.cc:159-177) over the caller's image points (n x 2), un-projected on the host with the same
// camera_unproject as k_prepare (same operations, same bits; cam null: the points as they stand); -1 without a minimum field of view
double compute_max_focal_length(const double *xy, size_t n, const CameraParams *cam, double min_fov) {
    if (!(min_fov > 0))
        return -1.0;
    double max_coord = 0.0;
    for (size_t i = 0; i < n; ++i) {
        double x = xy[2 * i], y = xy[2 * i + 1];
        if (cam)
            camera_unproject(*cam, x, y, x, y);
        max_coord = std::max(max_coord, std::fabs(x));
        max_coord = std::max(max_coord, std::fabs(y));
    }
    return max_coord / std::tan((min_fov * M_PI / 180.0) / 2.0); // (focal_max_focal_length's expression)
}

#include "driver_focal.inc"
#include "driver_sfocal.inc"
#include "driver_group.inc"
#include "driver_focal_group.inc"

} // namespace

// =============================================================================================== C-ABI
extern "C" {

const char *pl_version(void) { return "poselib_amd 0.1 (gfx950)"; }
int pl_abi_version(void) { return PL_ABI_VERSION; }
const char *pl_last_error(void) { return g_err.c_str(); }

void pl_default_ransac_options(pl_ransac_options *o) {
    o->max_iterations = 100000;
    o->min_iterations = 1000;
    o->dyn_num_trials_mult = 3.0;
    o->success_prob = 0.9999;
    o->seed = 0;
    o->progressive_sampling = 0;
    o->score_initial_model = 0;
    o->max_prosac_iterations = 100000;
}
void pl_default_bundle_options(pl_bundle_options *o) {
    std::memset(o, 0, sizeof(*o));
    o->max_iterations = 100;
    o->loss_type = LOSS_CAUCHY;
    o->lambda_update = 0;
    o->damping = 0;
    o->loss_scale = 1.0;
    o->gradient_tol = 1e-12;
    o->step_tol = 1e-8;
    o->relative_cost_tol = 1e-10;
    o->initial_lambda = 1e-3;
    o->min_lambda = 1e-10;
    o->max_lambda = 1e10;
    o->lambda_factor = 10.0;
}
void pl_default_robust_options(pl_robust_options *o, int kind) {
    std::memset(o, 0, sizeof(*o));
    pl_default_ransac_options(&o->ransac);
    pl_default_bundle_options(&o->bundle);
    o->max_error = (kind == 0 || kind == EST_RAD1D) ? 12.0 : 1.0;
    o->min_fov = 5.0; // types.h:126
}

int pl_set_lm_mode(int mode) {
    const int prev = pl::get_lm_mode();
    pl::set_lm_mode(mode);
    return prev;
}

int pl_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess)
        return 0;
    return n;
}
int pl_set_device(int device) {
    g_requested_device = device;
    Context *c;
    return get_context(&c);
}

int pl_problem_create(int kind, const double *a, const double *b, size_t n, pl_problem **out) {
    Context *c;
    int rc = get_context(&c);
    if (rc != PL_OK)
        return rc;
    pl_problem *p = new pl_problem();
    rc = make_problem(c, kind, a, b, n, p);
    if (rc != PL_OK) {
        delete p;
        return rc;
    }
    *out = p;
    return PL_OK;
}
// A resident tangent-Sampson problem (EST_RELT): bearings and un-projection Jacobians of the two images' pixels, computed on the
// device (k_prepare mode 3).  The pixels and cameras are taken as they stand - the ransac_relpose(x1, x2, cam1, cam2, ...) level of
// the reference, behind the rescaling of estimate_relative_pose (robust.cc:256-265).
int pl_problem_create_tangent(const double *x1, const double *x2, size_t n, const pl_camera *camera1, const pl_camera *camera2,
                              pl_problem **out) {
    if (!out || ((!x1 || !x2) && n))
        return fail(PL_ERR_INVALID, "points / output pointer is null");
    if ((camera1 && !camera_supported(camera1)) || (camera2 && !camera_supported(camera2)))
        return fail(PL_ERR_UNSUPPORTED, "camera model outside the supported set (or too few parameters)");
    if (n > 0x7fffffffu / 18)
        return fail(PL_ERR_INVALID, "too many correspondences");
    Context *c;
    int rc = get_context(&c);
    if (rc != PL_OK)
        return rc;
    pl_problem *p = new pl_problem();
    p->kind = EST_RELT;
    p->device = c->device;
    p->n = (uint32_t)n;
    p->d_pts = nullptr;
    std::memset(&p->ps, 0, sizeof(p->ps));
    p->ps.n = (uint32_t)n;
    p->ps.xy_absmax = std::numeric_limits<float>::infinity();
    *out = p;
    if (n == 0)
        return PL_OK;
    PrepareArgs pa;
    std::memset(&pa, 0, sizeof(pa));
    pa.mode = 3;
    pa.cam1 = to_cam(camera1);
    pa.cam2 = to_cam(camera2);
    pa.scale = 1.0;
    const size_t raw = sizeof(double) * 2 * n;
    hipError_t e = c->raw_a.ensure(raw);
    if (e == hipSuccess)
        e = c->raw_b.ensure(raw);
    if (e == hipSuccess)
        e = hipMalloc((void **)&p->d_pts, sizeof(double) * 18 * n);
    if (e == hipSuccess)
        e = hipMemcpyAsync(c->raw_a.p, x1, raw, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(c->raw_b.p, x2, raw, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess)
        e = launch_prepare(c->raw_a.as<double>(), c->raw_b.as<double>(), (uint32_t)n, pa, p->d_pts, nullptr, c->stream);
    if (e == hipSuccess)
        e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        if (p->d_pts)
            (void)hipFree(p->d_pts);
        delete p;
        *out = nullptr;
        return fail(PL_ERR_HIP, "preparation of the tangent-Sampson problem", e);
    }
    p->ps.a[0] = p->d_pts;
    return PL_OK;
}
// Diagnostic: correspondences per chunk of the tangent-Sampson streaming scorer as built (tests probe the sizes around it)
int pl_debug_tangent_chunk(void) { return tangent_score_chunk(); }
// Diagnostic: hypothesis slices of one member of a grouped scorer launch (driver_group.inc: group_score_slices).  No device call.
int pl_debug_group_slices(int kind, uint32_t n_points, uint32_t iterations, uint32_t launch_chunks) {
    if (!(kind == EST_ABS || kind == EST_REL || kind == EST_FUND || kind == EST_HOM || kind == EST_RAD1D) || n_points == 0 ||
        iterations == 0 || iterations > (1u << 30))
        return fail(PL_ERR_INVALID, "pl_debug_group_slices: kind 0, 1, 2, 3 or 5, n_points > 0, 0 < iterations <= 2^30");
    return debug_group_slices(kind, n_points, iterations, launch_chunks);
}
// Diagnostic: the inlier mask of one model on a resident problem, as the estimators' final get_inliers computes it (k_mask).
int pl_debug_inlier_mask(pl_problem *p, const void *model, double max_error, uint8_t *mask) {
    if (!p || !model || (!mask && p->n))
        return fail(PL_ERR_INVALID, "problem / model / mask pointer is null");
    Context *c;
    int rc = get_context(&c);
    if (rc != PL_OK)
        return rc;
    if (p->device != c->device)
        return fail(PL_ERR_INVALID, "problem lives on another device than the calling thread's");
    if (p->n == 0)
        return PL_OK;
    double rec[kModelStride];
    if (p->kind == EST_ABS || p->kind == EST_REL || p->kind == EST_RELT || p->kind == EST_RAD1D)
        record_from_pose(static_cast<const pl_camera_pose *>(model), p->kind == EST_REL || p->kind == EST_RELT, rec);
    else
        store_matrix_model(rec, mat_from_colmajor(static_cast<const double *>(model)));
    HIP_TRY(c->tmp_model.ensure(sizeof(double) * kModelStride));
    HIP_TRY(c->mask.ensure(p->n));
    HIP_TRY(hipMemcpyAsync(c->tmp_model.p, rec, sizeof(rec), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(launch_mask(p->kind, p->ps, c->tmp_model.as<double>(), max_error * max_error, c->mask.as<uint8_t>(), nullptr, c->stream));
    HIP_TRY(hipMemcpyAsync(mask, c->mask.p, p->n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(wait_stream(c));
    return PL_OK;
}
void pl_problem_destroy(pl_problem *p) {
    if (!p)
        return;
    free_problem(p);
    delete p;
}
int pl_ransac_run(pl_problem *p, const pl_robust_options *opt, void *model, uint8_t *inliers, pl_ransac_stats *stats) {
    if (!p || !model)
        return fail(PL_ERR_INVALID, "problem / model pointer is null");
    int rc = validate_options(opt);
    if (rc != PL_OK)
        return rc;
    Context *c;
    rc = get_context(&c);
    if (rc != PL_OK)
        return rc;
    if (p->device != c->device)
        return fail(PL_ERR_INVALID, "problem lives on another device than the calling thread's");
    pl_ransac_stats local;
    return run_with_model(c, p, opt, model, inliers, stats ? stats : &local);
}

int pl_ransac_run_sharded(pl_problem *p, const pl_robust_options *opt, const pl_shard *shard, void *model,
                          uint8_t *inliers, pl_ransac_stats *stats) {
    if (!shard || shard->world < 1 || shard->rank < 0 || shard->rank >= shard->world)
        return fail(PL_ERR_INVALID, "shard: need 0 <= rank < world");
    if (shard->world > 1 && !shard->allgather)
        return fail(PL_ERR_INVALID, "shard: all-gather callback missing");
    if (p && p->kind == EST_RAD1D)
        return fail(PL_ERR_UNSUPPORTED, "1D-radial problems (kind 5) are not served by the sharded run");
    g_shard = shard;
    const int rc = pl_ransac_run(p, opt, model, inliers, stats);
    g_shard = nullptr;
    return rc;
}

int pl_score_model(pl_problem *p, const void *model, double max_error, uint64_t *inlier_count, double *score) {
    if (!p || !model)
        return fail(PL_ERR_INVALID, "problem / model pointer is null");
    Context *c;
    int rc = get_context(&c);
    if (rc != PL_OK)
        return rc;
    if (p->device != c->device)
        return fail(PL_ERR_INVALID, "problem lives on another device than the calling thread's");
    double rec[kModelStride];
    if (p->kind == EST_ABS || p->kind == EST_REL || p->kind == EST_RELT || p->kind == EST_RAD1D)
        record_from_pose(static_cast<const pl_camera_pose *>(model), p->kind == EST_REL || p->kind == EST_RELT, rec);
    else
        store_matrix_model(rec, mat_from_colmajor(static_cast<const double *>(model)));
    HIP_TRY(c->tmp_model.ensure(sizeof(double) * kModelStride));
    HIP_TRY(hipMemcpyAsync(c->tmp_model.p, rec, sizeof(rec), hipMemcpyHostToDevice, c->stream));
    rc = enqueue_score_records(c, p, c->tmp_model.as<double>(), 1, max_error * max_error);
    if (rc != PL_OK)
        return rc;
    HIP_TRY(wait_stream(c));
    if (inlier_count)
        *inlier_count = c->h_count.as<uint32_t>()[0];
    if (score)
        *score = c->h_score.as<double>()[0];
    return PL_OK;
}

// Diagnostic: an arbitrary list of models through the STREAMING scorer of the main loop (k_gather_models -> k_live_list / k_gather_shadow16 ->
// k_score_mfma / k_score_queue -> k_finalize2), i.e. through the conservative pre-filters, instead of the sequential
// scorer pl_score_model uses.  Lets tests feed adversarial models / points to the filters on the device.
namespace {
// the caller's models as records in list order (pl_camera_pose[n] or double[n][9] column-major)
void debug_score_records(const pl_problem *p, const void *models, uint32_t H, std::vector<double> &recs) {
    const bool pose_kind = (p->kind == EST_ABS || p->kind == EST_REL || p->kind == EST_RELT || p->kind == EST_RAD1D);
    recs.assign((size_t)H * kModelStride, 0.0);
    for (uint32_t k = 0; k < H; ++k) {
        if (pose_kind)
            record_from_pose(static_cast<const pl_camera_pose *>(models) + k, p->kind == EST_REL || p->kind == EST_RELT, &recs[(size_t)k * kModelStride]);
        else
            store_matrix_model(&recs[(size_t)k * kModelStride], mat_from_colmajor(static_cast<const double *>(models) + 9 * (size_t)k));
    }
}
// What the generator, the compaction and the operand kernels of a batch step leave for the scorer, for a list the host wrote: the
// records in `b.models` in list order, the hypothesis-ordered copies, and the fp16 operands (absolute pose: live list, rank and the
// correspondences' rows as well) of the scorer `a` was wired for.  The partials are set to all-ones first: a (chunk, hypothesis)
// entry no wavefront writes then reads as a count of 2^32 - 1 and a NaN score, whatever an earlier launch left there.
int debug_score_prepare(Context *c, const pl_problem *p, const GroupArgs &a, const BatchBuffers &b, const BatchSizes &z,
                        const std::vector<double> &recs, const std::vector<uint32_t> &ident, uint32_t H) {
    BatchCtl hc;
    std::memset(&hc, 0, sizeof(hc));
    hc.num_hyp = H;
    HIP_TRY(hipMemsetAsync(b.ctl, 0, z.ctl, c->stream));
    HIP_TRY(hipMemcpyAsync(b.ctl, &hc, sizeof(hc), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(b.models, recs.data(), sizeof(double) * recs.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(b.slots, ident.data(), sizeof(uint32_t) * H, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(b.part_count, 0xff, z.part_count, c->stream));
    HIP_TRY(hipMemsetAsync(b.part_score, 0xff, z.part_score, c->stream));
    HIP_TRY(launch_gather_models(b.ctl, b.slots, b.models, H, b.shadow, b.compact64, c->stream));
    const Shadow16Params &s16 = a.comp.s16;
    if (s16.out && s16.sampson == 0) // as in the main loop: live list, operand rows of the live hypotheses and of the points
        HIP_TRY(launch_abs16(b.ctl, b.slots, b.models, H, p->ps, s16, c->stream));
    else if (s16.out && s16.sampson == 2)
        HIP_TRY(launch_hom16(b.ctl, b.slots, b.models, H, s16.thr, s16.out, c->stream));
    else if (s16.out)
        HIP_TRY(launch_sampson16(b.ctl, b.slots, b.models, H, s16.out, c->stream));
    return PL_OK;
}
// the single launch: slices_in 0 = the rule min(1536 / chunks, H) in workgroups of kScoreThreads, otherwise a grid of exactly
// slices_in workgroups of 8 wavefronts per chunk
int debug_score_single(pl_problem *p, const void *models, size_t n, double max_error, uint32_t slices_in, uint32_t *counts,
                       double *scores, int32_t *path_used, uint32_t *slices_used, uint32_t *chunks_used) {
    if (!p || (!models && n))
        return fail(PL_ERR_INVALID, "problem / models pointer is null");
    if (n > (1u << 22))
        return fail(PL_ERR_INVALID, "too many models");
    Context *c;
    int rc = get_context(&c);
    if (rc != PL_OK)
        return rc;
    if (p->device != c->device)
        return fail(PL_ERR_INVALID, "problem lives on another device than the calling thread's");
    if (path_used)
        *path_used = 0;
    if (slices_used)
        *slices_used = 0;
    if (chunks_used)
        *chunks_used = 0;
    const double thr2 = max_error * max_error;
    const PrefilterArgs pf = problem_prefilter(p, thr2);
    const bool use_mfma = score_uses_mfma(p->kind, p->n, pf);
    const uint32_t chunks = score_chunks(p->kind, p->n, true, use_mfma);
    if (slices_in > score_slice_limit(p->kind, chunks, use_mfma))
        return fail(PL_ERR_INVALID, "slices beyond what the scorer's launch takes for this problem");
    if (n == 0)
        return PL_OK;
    const uint32_t H = (uint32_t)n;
    if ((p->kind == EST_RELT || p->kind == EST_RAD1D) && p->n == 0) { // (no correspondence: no chunk to hold)
        for (uint32_t k = 0; k < H; ++k) {
            if (counts)
                counts[k] = 0;
            if (scores)
                scores[k] = 0.0;
        }
        return PL_OK;
    }
    std::vector<double> recs;
    std::vector<uint32_t> ident(H);
    for (uint32_t k = 0; k < H; ++k)
        ident[k] = k;
    debug_score_records(p, models, H, recs);
    // the buffers and arguments of a batch step whose H "iterations" hold one model each (no sampler: B = 0): the scorer's part of
    // them is used
    BatchRun run{};
    run.kind = p->kind;
    run.pts = p->ps;
    run.thr2 = thr2;
    run.pf = pf;
    BatchShape s{};
    s.Bl = H, s.slots = 1;
    s.use_mfma = use_mfma;
    s.chunks = chunks;
    s.point_rows = abs16_point_rows(p->n);
    const BatchSizes z = batch_step_sizes(p->kind, s);
    BatchBuffers bb;
    rc = context_batch_buffers(c, z, bb);
    if (rc != PL_OK)
        return rc;
    bb.nan_bits = nullptr; // (no generator: k_live_list reads the records' flag words)
    GroupArgs a;
    wire_batch_step(a, run, s, bb);
    rc = debug_score_prepare(c, p, a, bb, z, recs, ident, H);
    if (rc != PL_OK)
        return rc;
    const int path = a.comp.s16.out ? 2 : (run.pf.enabled ? 1 : 0);
    // launch_score counts slices in workgroups of kScoreThreads; the streaming kernels run 8 wavefronts per workgroup
    const uint32_t per = (uint32_t)kStreamWaves * 64u / (uint32_t)kScoreThreads;
    const uint32_t slices = slices_in ? slices_in * per : std::max<uint32_t>(1u, std::min<uint32_t>(1536u / s.chunks, H));
    HIP_TRY(launch_score(p->kind, a.score, slices, c->stream));
    HIP_TRY(launch_finalize(a.rec.f, c->stream));
    if (counts)
        HIP_TRY(hipMemcpyAsync(counts, c->count.p, sizeof(uint32_t) * H, hipMemcpyDeviceToHost, c->stream));
    if (scores)
        HIP_TRY(hipMemcpyAsync(scores, c->score.p, sizeof(double) * H, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(wait_stream(c));
    if (path_used)
        *path_used = path;
    if (slices_used)
        *slices_used = std::max<uint32_t>(1u, slices / per);
    if (chunks_used)
        *chunks_used = chunks;
    return PL_OK;
}
constexpr size_t kDebugScoreMembers = 4;
// The group form: a device-resident table whose slot 0 is inactive and whose slots 1 .. count hold the caller's members, every slot
// on an arena of its own (pack_batch_buffers), wired by wire_batch_step with the group's chunk shape, scored by launch_group_score
// and finished by launch_group_finalize_records - the two launches a group's batch step runs behind its operand kernels.
int debug_score_group(pl_debug_score_member *m, size_t count, uint32_t *idle_changed) {
    if (!m || count == 0 || count > kDebugScoreMembers)
        return fail(PL_ERR_INVALID, "the group form takes 1 .. 4 members");
    for (size_t i = 0; i < count; ++i) {
        if (!m[i].problem || !m[i].models || m[i].n == 0 || m[i].n > (1u << 22) || m[i].problem->n == 0)
            return fail(PL_ERR_INVALID, "member: problem / models missing, no correspondences, or n outside 1 .. 2^22");
        if (m[i].problem->kind != m[0].problem->kind)
            return fail(PL_ERR_INVALID, "the members of a group are of one kind");
    }
    const int kind = m[0].problem->kind;
    if (kind != EST_ABS && kind != EST_REL && kind != EST_FUND && kind != EST_HOM)
        return fail(PL_ERR_INVALID, "tangent and 1D-radial problems have no group form");
    Context *c;
    int rc = get_context(&c);
    if (rc != PL_OK)
        return rc;
    for (size_t i = 0; i < count; ++i)
        if (m[i].problem->device != c->device)
            return fail(PL_ERR_INVALID, "problem lives on another device than the calling thread's");
    struct Slot {
        BatchRun run{};
        BatchShape s{};
        BatchSizes z{};
        BatchBuffers b{};
        size_t bytes = 0;
        char *arena = nullptr;
        ~Slot() {
            if (arena)
                (void)hipFree(arena);
        }
    } slot[1 + kDebugScoreMembers];
    struct Scratch { // freed on every path
        void *p = nullptr;
        ~Scratch() {
            if (p)
                (void)hipFree(p);
        }
    } dtable;
    GroupArgs ha[1 + kDebugScoreMembers];
    GroupDims dims{};
    dims.G = (uint32_t)count + 1;
    dims.P = group_points_per_lane(kind);
    uint32_t launch_chunks = 0; // of the members k_score_mfma_g serves (run_group)
    for (size_t i = 0; i < count; ++i) {
        Slot &t = slot[i + 1];
        const pl_problem *p = m[i].problem;
        t.run.kind = kind;
        t.run.pts = p->ps;
        t.run.thr2 = m[i].max_error * m[i].max_error;
        t.run.pf = problem_prefilter(p, t.run.thr2);
        t.run.init_max = 0xffffffffu; // (no hypothesis improves on this: k_records_g lists none)
        t.s.Bl = (uint32_t)m[i].n, t.s.slots = 1;
        t.s.use_mfma = score_uses_mfma(kind, p->n, t.run.pf);
        t.s.chunks = group_member_chunks(kind, t.s.use_mfma, p->n);
        t.s.point_rows = t.s.chunks * 64u * (uint32_t)dims.P;
        if (m[i].slices > score_slice_limit(kind, t.s.chunks, false))
            return fail(PL_ERR_INVALID, "slices beyond what the scorer's launch takes for this member");
        t.z = batch_step_sizes(kind, t.s);
        if (t.s.use_mfma)
            launch_chunks += t.s.chunks;
    }
    slot[0].run = slot[1].run, slot[0].s = slot[1].s, slot[0].z = slot[1].z; // the inactive slot: a copy of the first member's
    for (size_t k = 0; k <= count; ++k) {
        Slot &t = slot[k];
        BatchBuffers unused;
        t.bytes = pack_batch_buffers(nullptr, t.z, unused);
        HIP_TRY(hipMalloc((void **)&t.arena, t.bytes));
        HIP_TRY(hipMemsetAsync(t.arena, k == 0 ? 0xa5 : 0, t.bytes, c->stream));
        pack_batch_buffers(t.arena, t.z, t.b);
        t.b.nan_bits = nullptr; // (no generator: k_live_list reads the records' flag words)
        t.b.host_meta = nullptr, t.b.host_models = nullptr, t.b.host_ctl = nullptr;
        wire_batch_step(ha[k], t.run, t.s, t.b);
    }
    ha[0].active = 0;
    for (size_t i = 0; i < count; ++i) {
        GroupArgs &a = ha[i + 1];
        const Slot &t = slot[i + 1];
        const uint32_t H = t.s.Bl;
        a.slices = m[i].slices ? m[i].slices
                               : group_score_slices(kind, t.s.use_mfma, group_expected_hypotheses(kind, H, H), H, t.s.chunks, launch_chunks);
        dims.max_B = std::max(dims.max_B, H);
        dims.max_hcap = std::max(dims.max_hcap, a.score.hyp_capacity);
        dims.max_chunks = std::max(dims.max_chunks, a.chunks);
        dims.max_slices = std::max(dims.max_slices, a.slices);
        dims.any_mfma |= a.use_mfma;
        dims.any_queue |= a.use_mfma ? 0u : 1u;
        std::vector<double> recs;
        std::vector<uint32_t> ident(H);
        for (uint32_t k = 0; k < H; ++k)
            ident[k] = k;
        debug_score_records(m[i].problem, m[i].models, H, recs);
        rc = debug_score_prepare(c, m[i].problem, a, t.b, t.z, recs, ident, H);
        if (rc != PL_OK)
            return rc;
        HIP_TRY(hipStreamSynchronize(c->stream)); // (recs / ident leave scope)
    }
    ha[0].slices = ha[1].slices;
    HIP_TRY(hipMalloc(&dtable.p, sizeof(GroupArgs) * dims.G));
    HIP_TRY(hipMemcpyAsync(dtable.p, ha, sizeof(GroupArgs) * dims.G, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(launch_group_score(kind, static_cast<const GroupArgs *>(dtable.p), dims, c->stream));
    HIP_TRY(launch_group_finalize_records(static_cast<const GroupArgs *>(dtable.p), dims, c->stream));
    for (size_t i = 0; i < count; ++i) {
        const Slot &t = slot[i + 1];
        if (m[i].counts)
            HIP_TRY(hipMemcpyAsync(m[i].counts, t.b.count, sizeof(uint32_t) * t.s.Bl, hipMemcpyDeviceToHost, c->stream));
        if (m[i].scores)
            HIP_TRY(hipMemcpyAsync(m[i].scores, t.b.score, sizeof(double) * t.s.Bl, hipMemcpyDeviceToHost, c->stream));
    }
    std::vector<uint32_t> idle(slot[0].bytes / 4);
    HIP_TRY(hipMemcpyAsync(idle.data(), slot[0].arena, idle.size() * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(wait_stream(c));
    uint32_t changed = 0;
    for (uint32_t w : idle)
        changed += w != 0xa5a5a5a5u ? 1u : 0u;
    if (idle_changed)
        *idle_changed = changed;
    for (size_t i = 0; i < count; ++i) {
        m[i].path_used = ha[i + 1].comp.s16.out ? 2 : (slot[i + 1].run.pf.enabled ? 1 : 0);
        m[i].slices_used = ha[i + 1].slices;
        m[i].chunks = ha[i + 1].chunks;
    }
    return PL_OK;
}
// The pruned form of the matrix-core absolute-pose scorer (PruneArgs) on lists the caller wrote, whatever score_prune_gate says of
// their length: route 0 - launch_score_pruned and launch_finalize_records, the launches of RansacRun::enqueue_batch, on the single
// launch's chunk shape; route 2 - a table with an inactive slot 0 through launch_group_score and launch_group_finalize_records, on
// the group's chunk shape.  Every slot has an arena of its own, as in debug_score_group.
// survivors (pl_debug_score_survivors): the count launch alone, over the whole list and every chunk; survivors[i] takes member i's
// [chunks][n] counts (hypothesis order, a NaN model reports 0), *guard_changed the words behind the live list's end that changed.
// bounded (pl_debug_score_bounded): the production sequence, bound tier included (PruneArgs.bound), no labels; per hypothesis the
// tier's bounds (no bound: 0xffffffff / NaN) and what became of it; columns (pl_debug_score_bounded_columns): the words of the count
// columns as the sequence left them.
struct DebugBoundedOut {
    uint32_t *const *bound_counts;
    double *const *bound_scores;
    uint8_t *const *tiers;
    uint32_t *const *columns = nullptr; // optional: [chunks][n] per member
};
int debug_score_pruned(int route, pl_debug_prune_member *m, size_t count, uint32_t *idle_changed, uint32_t *const *survivors = nullptr,
                       uint32_t *guard_changed = nullptr, const DebugBoundedOut *bounded = nullptr) {
    if (route != 0 && route != 2)
        return fail(PL_ERR_INVALID, "route: 0 single launch, 2 group form");
    if (!m || count == 0 || count > (route == 0 ? 1 : kDebugScoreMembers))
        return fail(PL_ERR_INVALID, "the single launch takes one member, the group form 1 .. 4");
    for (size_t i = 0; i < count; ++i) {
        if (!m[i].problem || !m[i].models || m[i].n == 0 || m[i].n > (1u << 22) || m[i].problem->n == 0)
            return fail(PL_ERR_INVALID, "member: problem / models missing, no correspondences, or n outside 1 .. 2^22");
        if (m[i].problem->kind != EST_ABS)
            return fail(PL_ERR_INVALID, "the pruned scorer is the absolute-pose one");
        if (m[i].cand_cap && !m[i].cand)
            return fail(PL_ERR_INVALID, "member: cand_cap without cand");
    }
    Context *c;
    int rc = get_context(&c);
    if (rc != PL_OK)
        return rc;
    for (size_t i = 0; i < count; ++i)
        if (m[i].problem->device != c->device)
            return fail(PL_ERR_INVALID, "problem lives on another device than the calling thread's");
    struct Slot {
        BatchRun run{};
        BatchShape s{};
        BatchSizes z{};
        BatchBuffers b{};
        size_t bytes = 0;
        char *arena = nullptr;
        ~Slot() {
            if (arena)
                (void)hipFree(arena);
        }
    } slot[1 + kDebugScoreMembers];
    struct Scratch { // freed on every path
        void *p = nullptr;
        ~Scratch() {
            if (p)
                (void)hipFree(p);
        }
    } dtable, dbound[kDebugScoreMembers];
    GroupArgs ha[1 + kDebugScoreMembers];
    GroupDims dims{};
    dims.G = (uint32_t)count + 1;
    dims.P = group_points_per_lane(EST_ABS);
    uint32_t launch_chunks = 0;
    for (size_t i = 0; i < count; ++i) {
        Slot &t = slot[i + 1];
        const pl_problem *p = m[i].problem;
        t.run.kind = EST_ABS;
        t.run.pts = p->ps;
        t.run.thr2 = m[i].max_error * m[i].max_error;
        t.run.pf = problem_prefilter(p, t.run.thr2);
        t.run.init_max = m[i].init_max;
        t.run.init_min = m[i].init_min;
        t.s.Bl = (uint32_t)m[i].n, t.s.slots = 1;
        t.s.use_mfma = score_uses_mfma(EST_ABS, p->n, t.run.pf);
        if (!t.s.use_mfma)
            return fail(PL_ERR_UNSUPPORTED, "member: not scored on the matrix cores (size, threshold or coordinates out of range)");
        if (route == 0) {
            t.s.chunks = score_chunks(EST_ABS, p->n, true, true);
            t.s.point_rows = abs16_point_rows(p->n);
        } else {
            t.s.chunks = group_member_chunks(EST_ABS, true, p->n);
            t.s.point_rows = t.s.chunks * 64u * (uint32_t)dims.P;
        }
        t.s.prune = true;
        t.z = batch_step_sizes(EST_ABS, t.s);
        launch_chunks += t.s.chunks;
    }
    slot[0].run = slot[1].run, slot[0].s = slot[1].s, slot[0].z = slot[1].z; // the inactive slot: a copy of the first member's
    for (size_t k = (route == 0 ? 1 : 0); k <= count; ++k) {
        Slot &t = slot[k];
        BatchBuffers unused;
        t.bytes = pack_batch_buffers(nullptr, t.z, unused);
        HIP_TRY(hipMalloc((void **)&t.arena, t.bytes));
        HIP_TRY(hipMemsetAsync(t.arena, k == 0 ? 0xa5 : 0, t.bytes, c->stream));
        pack_batch_buffers(t.arena, t.z, t.b);
        t.b.nan_bits = nullptr; // (no generator: k_live_list reads the records' flag words)
        t.b.host_meta = nullptr, t.b.host_models = nullptr, t.b.host_ctl = nullptr;
        wire_batch_step(ha[k], t.run, t.s, t.b);
        ha[k].score.prune.bound = bounded ? 1u : 0u;
        if (bounded && k > 0) { // the tier's sums per live position: scores, then count words; 0xff = none written
            const size_t hcap = ha[k].score.hyp_capacity;
            HIP_TRY(hipMalloc(&dbound[k - 1].p, hcap * 16));
            HIP_TRY(hipMemsetAsync(dbound[k - 1].p, 0xff, hcap * 16, c->stream));
            ha[k].score.prune.bnd_score = static_cast<double *>(dbound[k - 1].p);
            ha[k].score.prune.bnd_count = reinterpret_cast<uint32_t *>(ha[k].score.prune.bnd_score + hcap);
        }
    }
    ha[0].active = 0;
    for (size_t i = 0; i < count; ++i) {
        GroupArgs &a = ha[i + 1];
        const Slot &t = slot[i + 1];
        const uint32_t H = t.s.Bl;
        a.slices = group_score_slices(EST_ABS, true, group_expected_hypotheses(EST_ABS, H, H), H, t.s.chunks, launch_chunks);
        dims.max_B = std::max(dims.max_B, H);
        dims.max_hcap = std::max(dims.max_hcap, a.score.hyp_capacity);
        dims.max_chunks = std::max(dims.max_chunks, a.chunks);
        dims.max_slices = std::max(dims.max_slices, a.slices);
        dims.any_mfma = dims.any_prune = 1;
        dims.any_bound = bounded ? 1u : 0u;
        std::vector<double> recs;
        std::vector<uint32_t> ident(H);
        for (uint32_t k = 0; k < H; ++k)
            ident[k] = k;
        debug_score_records(m[i].problem, m[i].models, H, recs);
        rc = debug_score_prepare(c, m[i].problem, a, t.b, t.z, recs, ident, H);
        if (rc != PL_OK)
            return rc;
        HIP_TRY(hipStreamSynchronize(c->stream)); // (recs / ident leave scope)
    }
    uint32_t single_slices = 0;
    if (route == 0) {
        const GroupArgs &a = ha[1];
        const uint32_t slices = std::max<uint32_t>(1u, std::min<uint32_t>(1536u / a.chunks, a.score.hyp_capacity)); // enqueue_batch's
        single_slices = std::max<uint32_t>(1u, std::min<uint32_t>(slices * (uint32_t)kScoreThreads / (64u * (uint32_t)kStreamWaves),
                                                                  score_slice_limit(EST_ABS, a.chunks, true))); // (launch_score_pruned's grid)
        if (survivors) {
            HIP_TRY(launch_score_count(a.score, slices, c->stream));
        } else {
            HIP_TRY(launch_score_pruned(a.score, slices, c->stream));
            if (!bounded)
                HIP_TRY(launch_prune_label(a.score, c->stream));
            HIP_TRY(launch_finalize_records(a.rec, c->stream));
        }
    } else {
        ha[0].slices = ha[1].slices;
        HIP_TRY(hipMalloc(&dtable.p, sizeof(GroupArgs) * dims.G));
        HIP_TRY(hipMemcpyAsync(dtable.p, ha, sizeof(GroupArgs) * dims.G, hipMemcpyHostToDevice, c->stream));
        if (survivors) {
            HIP_TRY(launch_group_score_count(static_cast<const GroupArgs *>(dtable.p), dims, c->stream));
        } else {
            HIP_TRY(launch_group_score(EST_ABS, static_cast<const GroupArgs *>(dtable.p), dims, c->stream));
            // (the production step does not label: k_finalize2 needs dropped / not dropped alone)
            for (size_t i = 0; i < count && !bounded; ++i)
                HIP_TRY(launch_prune_label(ha[i + 1].score, c->stream));
            HIP_TRY(launch_group_finalize_records(static_cast<const GroupArgs *>(dtable.p), dims, c->stream));
        }
    }
    std::vector<std::vector<uint32_t>> part(count);
    std::vector<std::vector<uint32_t>> rank(count);
    std::vector<std::vector<uint8_t>> kept(count);
    std::vector<std::vector<RecordMeta>> meta(count);
    std::vector<PruneState> st(count);
    std::vector<BatchCtl> ctl(count);
    std::vector<std::vector<uint32_t>> bcount(count);
    std::vector<std::vector<double>> bscore(count);
    for (size_t i = 0; i < count; ++i) {
        const Slot &t = slot[i + 1];
        const uint32_t H = t.s.Bl;
        if (bounded) {
            const size_t hcap = ha[i + 1].score.hyp_capacity;
            bcount[i].resize(hcap), bscore[i].resize(hcap);
            HIP_TRY(hipMemcpyAsync(bcount[i].data(), ha[i + 1].score.prune.bnd_count, 4 * hcap, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipMemcpyAsync(bscore[i].data(), ha[i + 1].score.prune.bnd_score, 8 * hcap, hipMemcpyDeviceToHost, c->stream));
        }
        if (m[i].counts && !survivors)
            HIP_TRY(hipMemcpyAsync(m[i].counts, t.b.count, sizeof(uint32_t) * H, hipMemcpyDeviceToHost, c->stream));
        if (m[i].scores && !survivors)
            HIP_TRY(hipMemcpyAsync(m[i].scores, t.b.score, sizeof(double) * H, hipMemcpyDeviceToHost, c->stream));
        rank[i].resize(H), kept[i].resize(H), meta[i].resize(kRecordCap);
        HIP_TRY(hipMemcpyAsync(rank[i].data(), t.b.rank, sizeof(uint32_t) * H, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(kept[i].data(), t.b.prune_kept, H, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(meta[i].data(), t.b.rec_meta, sizeof(RecordMeta) * kRecordCap, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(&st[i], t.b.prune_state, sizeof(PruneState), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(&ctl[i], t.b.ctl, sizeof(BatchCtl), hipMemcpyDeviceToHost, c->stream));
        if (survivors || bounded) {
            part[i].resize((size_t)t.s.chunks * ha[i + 1].score.hyp_capacity);
            HIP_TRY(hipMemcpyAsync(part[i].data(), t.b.part_count, sizeof(uint32_t) * part[i].size(), hipMemcpyDeviceToHost, c->stream));
        }
    }
    std::vector<uint32_t> idle(route == 2 ? slot[0].bytes / 4 : 0);
    if (!idle.empty())
        HIP_TRY(hipMemcpyAsync(idle.data(), slot[0].arena, idle.size() * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(wait_stream(c));
    uint32_t changed = 0;
    for (uint32_t w : idle)
        changed += w != 0xa5a5a5a5u ? 1u : 0u;
    if (idle_changed)
        *idle_changed = changed;
    uint32_t guard = 0;
    for (size_t i = 0; i < count; ++i) {
        const uint32_t H = slot[i + 1].s.Bl, chunks = slot[i + 1].s.chunks;
        m[i].chunks = chunks;
        m[i].chunk_points = slot[i + 1].s.point_rows / chunks;
        m[i].num_live = ctl[i].num_live;
        m[i].slices = route == 0 ? single_slices : ha[i + 1].slices;
        if (survivors) { // (no lead, no selection, no finalize ran: every other field of the member stays as the caller left it)
            const uint32_t hcap = ha[i + 1].score.hyp_capacity;
            for (uint32_t ch = 0; ch < chunks; ++ch) {
                for (uint32_t k = 0; k < H; ++k)
                    survivors[i][(size_t)ch * H + k] = rank[i][k] == kNoRank ? 0u : part[i][(size_t)ch * hcap + rank[i][k]];
                for (uint32_t p = ctl[i].num_live; p < hcap; ++p) // (debug_score_prepare fills the partials with 0xff)
                    guard += part[i][(size_t)ch * hcap + p] != 0xffffffffu ? 1u : 0u;
            }
            continue;
        }
        if (bounded) {
            const uint32_t hcap = ha[i + 1].score.hyp_capacity;
            for (uint32_t ch = 0; ch < chunks; ++ch)
                for (uint32_t p = ctl[i].num_live; p < hcap; ++p)
                    guard += part[i][(size_t)ch * hcap + p] != 0xffffffffu ? 1u : 0u;
            for (uint32_t k = 0; k < H; ++k) { // 0 exact scores, 1 dropped on survivor counts, 2 dropped on bounds, 3 NaN model
                const uint32_t p = rank[i][k];
                const bool live = p != kNoRank;
                const bool has = live && bcount[i][p] != 0xffffffffu;
                bounded->bound_counts[i][k] = has ? bcount[i][p] : 0xffffffffu;
                bounded->bound_scores[i][k] = has ? bscore[i][p] : std::numeric_limits<double>::quiet_NaN();
                bounded->tiers[i][k] = !live ? 3 : kept[i][p] == kKept ? 0 : has ? 2 : 1;
                for (uint32_t ch = 0; bounded->columns && ch < chunks; ++ch)
                    bounded->columns[i][(size_t)ch * H + k] = live ? part[i][(size_t)ch * hcap + p] : 0u;
            }
        }
        const bool split = st[i].cstar < chunks; // (otherwise nothing was dropped or pruned)
        // kept = the exact rule: the pre-selected positions that k_prune_label left alone
        uint32_t selected = 0;
        for (uint32_t k = 0; k < H; ++k) {
            const bool live = rank[i][k] != kNoRank;
            const bool kp = !split || !live || kept[i][rank[i][k]] == kKept;
            selected += (split && live && kp) ? 1u : 0u;
            if (m[i].kept)
                m[i].kept[k] = kp ? 1 : 0;
        }
        m[i].num_cand = ctl[i].num_records;
        for (uint32_t r = 0; r < std::min<uint32_t>({ctl[i].num_records, m[i].cand_cap, kRecordCap}); ++r)
            m[i].cand[r] = meta[i][r].k;
        m[i].cstar = st[i].cstar;
        m[i].lead = kPruneLead;
        m[i].lead_max = st[i].lead_max;
        m[i].lead_min = st[i].lead_min;
        m[i].num_selected = selected;
        m[i].num_preselected = st[i].sel_len;
    }
    if (guard_changed)
        *guard_changed = guard;
    return PL_OK;
}
} // namespace
int pl_debug_score_pruned(int route, pl_debug_prune_member *members, size_t num_members, uint32_t *idle_changed) {
    if (idle_changed)
        *idle_changed = 0;
    return debug_score_pruned(route, members, num_members, idle_changed);
}
int pl_debug_score_survivors(int route, pl_debug_prune_member *members, size_t num_members, uint32_t *const *survivors,
                             uint32_t *idle_changed, uint32_t *guard_changed) {
    if (idle_changed)
        *idle_changed = 0;
    if (guard_changed)
        *guard_changed = 0;
    if (!survivors)
        return fail(PL_ERR_INVALID, "pl_debug_score_survivors: survivors missing");
    for (size_t i = 0; i < num_members; ++i)
        if (!survivors[i])
            return fail(PL_ERR_INVALID, "pl_debug_score_survivors: a member without an output array");
    return debug_score_pruned(route, members, num_members, idle_changed, survivors, guard_changed);
}
int pl_debug_score_bounded(int route, pl_debug_prune_member *members, size_t num_members, uint32_t *const *bound_counts,
                           double *const *bound_scores, uint8_t *const *tiers, uint32_t *idle_changed, uint32_t *guard_changed) {
    if (idle_changed)
        *idle_changed = 0;
    if (guard_changed)
        *guard_changed = 0;
    if (!bound_counts || !bound_scores || !tiers)
        return fail(PL_ERR_INVALID, "pl_debug_score_bounded: output arrays missing");
    for (size_t i = 0; i < num_members; ++i)
        if (!bound_counts[i] || !bound_scores[i] || !tiers[i])
            return fail(PL_ERR_INVALID, "pl_debug_score_bounded: a member without an output array");
    const DebugBoundedOut out{bound_counts, bound_scores, tiers};
    return debug_score_pruned(route, members, num_members, idle_changed, nullptr, guard_changed, &out);
}
int pl_debug_score_bounded_columns(int route, pl_debug_prune_member *members, size_t num_members, uint32_t *const *bound_counts,
                                   double *const *bound_scores, uint8_t *const *tiers, uint32_t *const *columns, uint32_t *idle_changed,
                                   uint32_t *guard_changed) {
    if (idle_changed)
        *idle_changed = 0;
    if (guard_changed)
        *guard_changed = 0;
    if (!bound_counts || !bound_scores || !tiers || !columns)
        return fail(PL_ERR_INVALID, "pl_debug_score_bounded_columns: output arrays missing");
    for (size_t i = 0; i < num_members; ++i)
        if (!bound_counts[i] || !bound_scores[i] || !tiers[i] || !columns[i])
            return fail(PL_ERR_INVALID, "pl_debug_score_bounded_columns: a member without an output array");
    const DebugBoundedOut out{bound_counts, bound_scores, tiers, columns};
    return debug_score_pruned(route, members, num_members, idle_changed, nullptr, guard_changed, &out);
}
int pl_debug_score_prune_gate(int kind, uint32_t n_points, uint32_t iterations) {
    PrefilterArgs pf{}; // as pl_debug_group_slices: a prefilter in range is assumed
    pf.enabled = 1;
    pf.g16 = pf.t16 = pf.h16 = 1.0f, pf.thr = 1.0f;
    if (n_points == 0)
        return fail(PL_ERR_INVALID, "pl_debug_score_prune_gate: n_points > 0");
    const bool mfma = score_uses_mfma(kind, n_points, pf);
    return score_prune_gate(kind, mfma, iterations, kind == EST_ABS ? score_chunks(kind, n_points, true, mfma) : 1u) ? 1 : 0;
}
int pl_debug_lm_route(int kind, uint32_t n_points, uint64_t max_iterations, uint32_t *slices) {
    const bool known = kind == EST_ABS || kind == EST_REL || kind == EST_FUND || kind == EST_HOM || kind == EST_RELT || kind == EST_RAD1D;
    if (!known || n_points == 0 || !slices)
        return fail(PL_ERR_INVALID, "pl_debug_lm_route: kind 0 .. 5, n_points > 0, slices pointer");
    const LMRoute r = lm_route(kind, n_points, true, (uint32_t)std::min<uint64_t>(max_iterations, 0xffffffffu)); // (to_lm's clamp)
    *slices = r.slices;
    return r.kernel;
}
int pl_debug_score_stream(pl_problem *p, const void *models, size_t n, double max_error, uint32_t *counts,
                          double *scores, int32_t *path_used) {
    return debug_score_single(p, models, n, max_error, 0, counts, scores, path_used, nullptr, nullptr);
}
// Diagnostic: pl_debug_score_stream with the scorer's grid in the caller's hand (route 0, one member), and the group form of the same
// kernels (route 2, up to four members behind an inactive slot); the header states the contract.
int pl_debug_score_stream_ex(int route, pl_debug_score_member *members, size_t num_members, uint32_t *idle_changed) {
    if (idle_changed)
        *idle_changed = 0;
    if (route != 0 && route != 2)
        return fail(PL_ERR_INVALID, "route: 0 single launch, 2 group form");
    if (route == 2)
        return debug_score_group(members, num_members, idle_changed);
    if (!members || num_members != 1)
        return fail(PL_ERR_INVALID, "the single launch takes one member");
    pl_debug_score_member &m = members[0];
    return debug_score_single(m.problem, m.models, m.n, m.max_error, m.slices, m.counts, m.scores, &m.path_used, &m.slices_used, &m.chunks);
}
// Diagnostic: chunks of correspondences and points per lane of the streaming scorers, as score_shape (single launch) or
// group_member_chunks (group form) cut a problem.  No device call.
int pl_debug_score_shape(int kind, uint32_t n_points, int matrix_core, int group_form, uint32_t *chunks, uint32_t *points_per_lane) {
    const bool four = kind == EST_ABS || kind == EST_REL || kind == EST_FUND || kind == EST_HOM;
    if (!(four || kind == EST_RELT || kind == EST_RAD1D) || n_points == 0 || !chunks || !points_per_lane)
        return fail(PL_ERR_INVALID, "pl_debug_score_shape: kind 0 .. 5, n_points > 0, output pointers");
    if (!four && (matrix_core || group_form))
        return fail(PL_ERR_INVALID, "tangent and 1D-radial problems have neither a matrix-core nor a group form");
    if (matrix_core) { // as pl_debug_group_slices: the prefilter of a problem with in-range coordinates and threshold is assumed
        PrefilterArgs pf{};
        pf.enabled = 1;
        pf.g16 = pf.t16 = pf.h16 = 1.0f, pf.thr = 1.0f;
        if (!score_uses_mfma(kind, n_points, pf))
            return fail(PL_ERR_UNSUPPORTED, "no problem of this kind and size is scored on the matrix cores");
    }
    if (group_form) {
        *chunks = group_member_chunks(kind, matrix_core != 0, n_points);
        *points_per_lane = (uint32_t)((matrix_core && (kind == EST_REL || kind == EST_FUND)) ? group_mfma2_points_per_lane(kind)
                                                                                           : group_points_per_lane(kind));
    } else {
        *chunks = score_chunks(kind, n_points, true, matrix_core != 0);
        *points_per_lane = (uint32_t)score_points_per_lane(kind, n_points, true, matrix_core != 0);
    }
    return PL_OK;
}

// Diagnostic: the device sampler's window and the orbit kernel's builds, as the driver and the launchers compute them.  No device call.
int pl_debug_sampler_shape(int K, uint64_t N, uint32_t B, uint64_t window, pl_debug_sampler_shape_info *out) {
    if ((K != 3 && K != 4 && K != 5 && K != 7) || N < (uint64_t)K || N > 0xffffffffull || B == 0 || !out)
        return fail(PL_ERR_INVALID, "pl_debug_sampler_shape: K in {3, 4, 5, 7}, K <= N < 2^32, B > 0, output pointer");
    const uint64_t M = window ? window : sampler_window((uint32_t)N, K, B);
    const OrbitShape sm = orbit_build_shape(true), lg = orbit_build_shape(false);
    out->window = M;
    out->build = (M <= 0xffffffffull && orbit_small_build((uint32_t)M, N, K)) ? 1u : 2u;
    out->tile = sm.tile;
    out->small_flags = sm.flags, out->small_doubling = sm.doubling, out->small_segments = sm.segments;
    out->large_flags = lg.flags, out->large_doubling = lg.doubling, out->large_segments = lg.segments;
    return PL_OK;
}
// Diagnostic: the sampler's launches on their own (the header states the contract).  Every slot - the inactive one of the group form
// included - has an arena of its own that holds the four buffers the sampler touches, sized by batch_step_sizes and packed by
// pack_batch_buffers; the table entries are wire_batch_step's.
int pl_debug_sample_positions(int route, int K, int build, pl_debug_sampler_member *m, size_t count, uint32_t *idle_changed) {
    if (idle_changed)
        *idle_changed = 0;
    if (route != 0 && route != 2)
        return fail(PL_ERR_INVALID, "route: 0 single launches, 2 group form");
    if (build < 0 || build > 2)
        return fail(PL_ERR_INVALID, "build: 0 the launcher's choice, 1 small, 2 large");
    if (K != 3 && K != 4 && K != 5 && K != 7)
        return fail(PL_ERR_INVALID, "K: 3, 4, 5 or 7");
    constexpr size_t kMembers = 4;
    if (!m || count == 0 || count > kMembers)
        return fail(PL_ERR_INVALID, "1 .. 4 members");
    const int kind = K == 3 ? EST_ABS : K == 5 ? EST_REL : K == 7 ? EST_FUND : EST_HOM;
    uint64_t window[kMembers];
    for (size_t i = 0; i < count; ++i) {
        if (m[i].N < (uint64_t)K || m[i].N > 0xffffffffull || m[i].B == 0 || m[i].B > (1u << 20) || !m[i].positions)
            return fail(PL_ERR_INVALID, "member: K <= N < 2^32, B in 1 .. 2^20, positions");
        window[i] = m[i].M ? m[i].M : sampler_window((uint32_t)m[i].N, K, m[i].B);
        if (window[i] > 0x7fffffffull || m[i].pos_base + window[i] >= 0xffffffffull || m[i].pos_base >= 0xffffffffull) // (enqueue_batch's limits)
            return fail(PL_ERR_INVALID, "member: a window beyond 2^31 - 1 positions, or one that ends at or beyond draw 2^32 - 1");
        if (route == 2 && (m[i].planted != nullptr) != (m[0].planted != nullptr))
            return fail(PL_ERR_INVALID, "a group is drawn or planted as a whole");
    }
    Context *c;
    int rc = get_context(&c);
    if (rc != PL_OK)
        return rc;
    struct Slot {
        BatchRun run{};
        BatchShape s{};
        BatchSizes z{};
        BatchBuffers b{};
        size_t bytes = 0;
        char *arena = nullptr;
        ~Slot() {
            if (arena)
                (void)hipFree(arena);
        }
    } slot[1 + kMembers];
    struct Scratch { // freed on every path
        void *p = nullptr;
        ~Scratch() {
            if (p)
                (void)hipFree(p);
        }
    } dtable;
    GroupArgs ha[1 + kMembers];
    GroupDims dims{};
    dims.G = (uint32_t)count + 1;
    dims.min_n = 0xffffffffu;
    for (size_t i = 0; i < count; ++i) {
        Slot &t = slot[i + 1];
        t.run.kind = kind;
        t.run.pts.n = (uint32_t)m[i].N;
        t.run.seed = m[i].seed, t.run.pos = m[i].pos_base;
        t.s.B = t.s.Bl = m[i].B, t.s.M = (uint32_t)window[i], t.s.slots = 1, t.s.chunks = 1;
        const BatchSizes full = batch_step_sizes(kind, t.s);
        t.z.positions = full.positions, t.z.delta = full.delta, t.z.flags = full.flags, t.z.ctl = full.ctl; // (the sampler's buffers only)
    }
    slot[0].run = slot[1].run, slot[0].s = slot[1].s, slot[0].z = slot[1].z; // the inactive slot: a copy of the first member's
    std::vector<uint64_t> bits;
    for (size_t k = (route == 0 ? 1 : 0); k <= count; ++k) {
        Slot &t = slot[k];
        BatchBuffers unused;
        t.bytes = pack_batch_buffers(nullptr, t.z, unused);
        t.bytes += 256; // (the word behind the control block is read back, whatever the block's size)
        HIP_TRY(hipMalloc((void **)&t.arena, t.bytes));
        HIP_TRY(hipMemsetAsync(t.arena, 0xa5, t.bytes, c->stream));
        pack_batch_buffers(t.arena, t.z, t.b);
        t.b.host_meta = nullptr, t.b.host_models = nullptr, t.b.host_ctl = nullptr;
        wire_batch_step(ha[k], t.run, t.s, t.b);
        if (k == 0)
            continue;
        const pl_debug_sampler_member &mi = m[k - 1];
        group_dims_sampler(dims, t.s.M, t.run.pts.n, t.s.B);
        HIP_TRY(hipMemsetAsync(t.b.positions, 0xff, t.z.positions, c->stream));
        if (mi.planted) {
            const uint32_t M = t.s.M, words = (M + 63u) / 64u;
            bits.assign(words, 0ull);
            for (uint32_t p = 0; p < M; ++p)
                if (mi.planted[p] != (uint8_t)K)
                    bits[p >> 6] |= 1ull << (p & 63u);
            HIP_TRY(hipMemcpyAsync(t.b.delta, mi.planted, M, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(hipMemcpyAsync(t.b.flags, bits.data(), sizeof(uint64_t) * words, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(hipMemsetAsync(t.b.ctl, 0, t.z.ctl, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream)); // (`bits` is reused)
        }
    }
    const bool planted = m[0].planted != nullptr;
    uint32_t build_used[1 + kMembers] = {};
    if (route == 0) {
        for (size_t i = 0; i < count; ++i) {
            const SampleArgs &sa = ha[i + 1].samp;
            HIP_TRY(m[i].planted ? launch_sample_orbit(K, sa, c->stream, build) : launch_sample_positions(K, sa, c->stream, build));
            build_used[i + 1] = build ? (uint32_t)build : (orbit_small_build(sa.M, sa.N, K) ? 1u : 2u);
        }
    } else {
        ha[0].active = 0;
        HIP_TRY(hipMalloc(&dtable.p, sizeof(GroupArgs) * dims.G));
        HIP_TRY(hipMemcpyAsync(dtable.p, ha, sizeof(GroupArgs) * dims.G, hipMemcpyHostToDevice, c->stream));
        const GroupArgs *table = static_cast<const GroupArgs *>(dtable.p);
        HIP_TRY(planted ? launch_group_orbit(K, table, dims, c->stream, build) : launch_group_positions(K, table, dims, c->stream, build));
        for (size_t i = 0; i < count; ++i)
            build_used[i + 1] = build ? (uint32_t)build : (orbit_small_build(dims.max_M, dims.min_n, K) ? 1u : 2u);
    }
    std::vector<uint8_t> hdelta[kMembers];
    std::vector<uint64_t> hflags[kMembers];
    std::vector<uint32_t> hctl[kMembers];
    for (size_t i = 0; i < count; ++i) {
        const Slot &t = slot[i + 1];
        hdelta[i].resize(t.z.delta), hflags[i].resize(t.z.flags / sizeof(uint64_t)), hctl[i].resize(t.z.ctl / 4 + 1);
        HIP_TRY(hipMemcpyAsync(m[i].positions, t.b.positions, t.z.positions, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(hdelta[i].data(), t.b.delta, t.z.delta, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(hflags[i].data(), t.b.flags, t.z.flags, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(hctl[i].data(), t.b.ctl, sizeof(uint32_t) * hctl[i].size(), hipMemcpyDeviceToHost, c->stream));
    }
    std::vector<uint32_t> idle(route == 2 ? slot[0].bytes / 4 : 0);
    if (!idle.empty())
        HIP_TRY(hipMemcpyAsync(idle.data(), slot[0].arena, idle.size() * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(wait_stream(c));
    uint32_t changed = 0;
    for (uint32_t w : idle)
        changed += w != 0xa5a5a5a5u ? 1u : 0u;
    if (idle_changed)
        *idle_changed = changed;
    for (size_t i = 0; i < count; ++i) {
        const Slot &t = slot[i + 1];
        const uint32_t M = t.s.M;
        BatchCtl ctl;
        std::memcpy(&ctl, hctl[i].data(), sizeof(ctl));
        m[i].pos_after = ctl.pos_after;
        m[i].orbit_error = ctl.orbit_error;
        m[i].M_used = M;
        m[i].build_used = build_used[i + 1];
        if (m[i].delta)
            std::memcpy(m[i].delta, hdelta[i].data(), M);
        if (m[i].flagbits)
            std::memcpy(m[i].flagbits, hflags[i].data(), t.z.flags);
        bool guard = true;
        for (size_t k = M; k < hdelta[i].size(); ++k)
            guard = guard && hdelta[i][k] == 0xa5u;
        m[i].delta_guard = guard ? 1 : 0;
        ctl.pos_after = 0, ctl.orbit_error = 0;
        std::memcpy(hctl[i].data(), &ctl, sizeof(ctl));
        bool clear = hctl[i].back() == 0xa5a5a5a5u;
        for (size_t k = 0; k + 1 < hctl[i].size(); ++k)
            clear = clear && hctl[i][k] == 0u;
        m[i].ctl_clear = clear ? 1 : 0;
        m[i].pad = 0;
    }
    return PL_OK;
}

int pl_debug_device_math(int fn, const double *x, size_t n, double *out) {
    if (fn < 0 || fn >= kDeviceMathFns)
        return fail(PL_ERR_INVALID, "unknown device math function");
    if ((!x || !out) && n)
        return fail(PL_ERR_INVALID, "null pointer");
    if (n > (1u << 28))
        return fail(PL_ERR_INVALID, "too many values");
    Context *c;
    int rc = get_context(&c);
    if (rc != PL_OK)
        return rc;
    if (n == 0)
        return PL_OK;
    struct Scratch { // freed on every path
        void *p = nullptr;
        ~Scratch() {
            if (p)
                (void)hipFree(p);
        }
    } din, dout;
    HIP_TRY(hipMalloc(&din.p, sizeof(double) * n));
    HIP_TRY(hipMalloc(&dout.p, sizeof(double) * n));
    HIP_TRY(hipMemcpyAsync(din.p, x, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(launch_device_math(fn, static_cast<const double *>(din.p), (uint32_t)n, static_cast<double *>(dout.p), c->stream));
    HIP_TRY(hipMemcpyAsync(out, dout.p, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PL_OK;
}

int pl_debug_device_math2(int fn, const double *x, const double *y, size_t n, double *out) {
    if (fn < 0 || fn >= kDeviceMath2Fns)
        return fail(PL_ERR_INVALID, "unknown device math function");
    if ((!x || !out || (fn == 0 && !y)) && n)
        return fail(PL_ERR_INVALID, "null pointer");
    if (n > (1u << 28))
        return fail(PL_ERR_INVALID, "too many values");
    Context *c;
    int rc = get_context(&c);
    if (rc != PL_OK)
        return rc;
    if (n == 0)
        return PL_OK;
    struct Scratch { // freed on every path
        void *p = nullptr;
        ~Scratch() {
            if (p)
                (void)hipFree(p);
        }
    } dx, dy, dout;
    HIP_TRY(hipMalloc(&dx.p, sizeof(double) * n));
    HIP_TRY(hipMalloc(&dout.p, sizeof(double) * n));
    HIP_TRY(hipMemcpyAsync(dx.p, x, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    if (fn == 0) {
        HIP_TRY(hipMalloc(&dy.p, sizeof(double) * n));
        HIP_TRY(hipMemcpyAsync(dy.p, y, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    }
    HIP_TRY(launch_device_math2(fn, static_cast<const double *>(dx.p), static_cast<const double *>(fn == 0 ? dy.p : dx.p), (uint32_t)n,
                                static_cast<double *>(dout.p), c->stream));
    HIP_TRY(hipMemcpyAsync(out, dout.p, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PL_OK;
}

int pl_refine_model(pl_problem *p, const pl_bundle_options *opt, const pl_camera *camera, const uint8_t *mask,
                    void *model, uint32_t *lm_iterations) {
    if (!p || !model || !opt)
        return fail(PL_ERR_INVALID, "problem / options / model pointer is null");
    if (p->kind == EST_ABS && camera && active_cam_flags(to_cam(camera).model_id, *opt))
        return fail(PL_ERR_INVALID, "refine_* moves the camera: call pl_bundle_adjust_camera (camera in / out)");
    if (camera && !camera_supported(camera))
        return fail(PL_ERR_UNSUPPORTED, "camera model not supported (NULL, SIMPLE_PINHOLE, PINHOLE, SIMPLE_RADIAL, RADIAL, OPENCV, OPENCV_FISHEYE, SIMPLE_RADIAL_FISHEYE, RADIAL_FISHEYE)");
    Context *c;
    int rc = get_context(&c);
    if (rc != PL_OK)
        return rc;
    if (p->device != c->device)
        return fail(PL_ERR_INVALID, "problem lives on another device than the calling thread's");
    RefineJob j;
    const bool pose_kind = (p->kind == EST_ABS || p->kind == EST_REL || p->kind == EST_RELT || p->kind == EST_RAD1D);
    if (pose_kind)
        record_from_pose(static_cast<const pl_camera_pose *>(model), p->kind == EST_REL || p->kind == EST_RELT, j.record_in);
    else
        store_matrix_model(j.record_in, mat_from_colmajor(static_cast<const double *>(model)));
    j.opt = to_lm(*opt);
    j.cam = to_cam(camera);
    j.point_scale = 1.0;
    j.prefilter_thr2 = 0.0;
    j.d_mask = nullptr;
    if (mask && p->n) {
        HIP_TRY(c->mask.ensure(p->n));
        HIP_TRY(hipMemcpyAsync(c->mask.p, mask, p->n, hipMemcpyHostToDevice, c->stream));
        j.d_mask = c->mask.as<uint8_t>();
    }
    std::vector<RefineJob> jobs{j};
    rc = run_refinements(c, p, jobs, false, 0.0);
    if (rc != PL_OK)
        return rc;
    if (lm_iterations)
        *lm_iterations = c->h_tasks.as<LMTask>()[0].iterations;
    if (pose_kind) {
        pose_from_record(jobs[0].record_out, static_cast<pl_camera_pose *>(model));
    } else {
        Mat3 M;
        for (int i = 0; i < 9; ++i)
            M.m[i] = jobs[0].record_out[kMatOff + i];
        mat_to_colmajor(M, static_cast<double *>(model));
    }
    return PL_OK;
}

// bundle_adjust(x, X, Image *image, BundleOptions) (the Image overload, robust/bundle.cc:94-113) on an absolute-pose
// problem holding PIXEL coordinates: the pose and - per opt->refine_focal_length / refine_principal_point /
// refine_extra_params - the camera's intrinsics, both in / out.
int pl_bundle_adjust_camera(pl_problem *p, const pl_bundle_options *opt, pl_camera *camera, const uint8_t *mask,
                            pl_camera_pose *pose, uint32_t *lm_iterations) {
    if (!p || !pose || !opt || !camera)
        return fail(PL_ERR_INVALID, "problem / options / camera / pose pointer is null");
    if (p->kind != EST_ABS)
        return fail(PL_ERR_INVALID, "pl_bundle_adjust_camera refines absolute poses");
    if (!camera_supported(camera))
        return fail(PL_ERR_UNSUPPORTED, "camera model not supported (NULL, SIMPLE_PINHOLE, PINHOLE, SIMPLE_RADIAL, RADIAL, OPENCV, OPENCV_FISHEYE, SIMPLE_RADIAL_FISHEYE, RADIAL_FISHEYE)");
    Context *c;
    int rc = get_context(&c);
    if (rc != PL_OK)
        return rc;
    if (p->device != c->device)
        return fail(PL_ERR_INVALID, "problem lives on another device than the calling thread's");
    RefineJob j;
    record_from_pose(pose, false, j.record_in);
    j.opt = to_lm(*opt);
    j.cam = to_cam(camera);
    j.cam_flags = active_cam_flags(j.cam.model_id, *opt);
    j.point_scale = 1.0;
    j.prefilter_thr2 = 0.0;
    j.d_mask = nullptr;
    if (mask && p->n) {
        HIP_TRY(c->mask.ensure(p->n));
        HIP_TRY(hipMemcpyAsync(c->mask.p, mask, p->n, hipMemcpyHostToDevice, c->stream));
        j.d_mask = c->mask.as<uint8_t>();
    }
    std::vector<RefineJob> jobs{j};
    rc = run_refinements(c, p, jobs, false, 0.0);
    if (rc != PL_OK)
        return rc;
    if (lm_iterations)
        *lm_iterations = c->h_tasks.as<LMTask>()[0].iterations;
    pose_from_record(jobs[0].record_out, pose);
    if (j.cam_flags)
        for (int i = 0; i < camera->num_params && i < 12; ++i)
            camera->params[i] = jobs[0].cam_out.p[i];
    return PL_OK;
}

static int ransac_oneshot(int kind, const double *a, const double *b, size_t n, const pl_robust_options *opt,
                          void *model, uint8_t *inliers, pl_ransac_stats *stats) {
    int rc = validate_options(opt);
    if (rc != PL_OK)
        return rc;
    Context *c;
    rc = get_context(&c);
    if (rc != PL_OK)
        return rc;
    pl_problem p;
    rc = make_problem(c, kind, a, b, n, &p);
    if (rc != PL_OK)
        return rc;
    pl_ransac_stats local;
    rc = run_with_model(c, &p, opt, model, inliers, stats ? stats : &local);
    free_problem(&p);
    return rc;
}
int pl_ransac_pnp(const double *x, const double *X, size_t n, const pl_robust_options *opt, pl_camera_pose *pose,
                  uint8_t *inliers, pl_ransac_stats *stats) {
    return ransac_oneshot(EST_ABS, x, X, n, opt, pose, inliers, stats);
}
int pl_ransac_pnpf(const double *x, const double *X, size_t n, const pl_robust_options *opt, pl_camera_pose *pose, double *focal,
                   uint8_t *inliers, pl_ransac_stats *stats) {
    if (!opt || !pose || !focal)
        return fail(PL_ERR_INVALID, "null argument");
    pl_robust_options o = *opt;
    o.estimate_focal_length = 1;
    int rc = validate_options(&o, /*focal_entry=*/true);
    if (rc != PL_OK)
        return rc;
    Context *c;
    rc = get_context(&c);
    if (rc != PL_OK)
        return rc;
    pl_problem p;
    rc = make_problem(c, EST_ABS, x, X, n, &p);
    if (rc != PL_OK)
        return rc;
    pl_ransac_stats local;
    rc = run_focal(c, &p, &o, pose, focal, inliers, stats ? stats : &local, x, nullptr);
    free_problem(&p);
    return rc;
}
int pl_ransac_shared_focal_relpose(const double *x1, const double *x2, size_t n, const pl_robust_options *opt, pl_camera_pose *pose,
                                   double *focal, uint8_t *inliers, pl_ransac_stats *stats) {
    if (!opt || !pose || !focal)
        return fail(PL_ERR_INVALID, "null argument");
    int rc = validate_options(opt);
    if (rc != PL_OK)
        return rc;
    Context *c;
    rc = get_context(&c);
    if (rc != PL_OK)
        return rc;
    pl_problem p;
    rc = make_problem(c, EST_FUND, x1, x2, n, &p); // (two-view layout: x1, y1, x2, y2)
    if (rc != PL_OK)
        return rc;
    pl_ransac_stats local;
    rc = run_shared_focal(c, &p, opt, pose, focal, inliers, stats ? stats : &local);
    free_problem(&p);
    return rc;
}
int pl_refine_shared_focal_relpose(const double *x1, const double *x2, size_t n, const pl_bundle_options *opt, pl_camera_pose *pose,
                                   double *focal, uint32_t *lm_iterations) {
    if (!opt || !pose || !focal)
        return fail(PL_ERR_INVALID, "null argument");
    Context *c;
    int rc = get_context(&c);
    if (rc != PL_OK)
        return rc;
    pl_problem p;
    rc = make_problem(c, EST_FUND, x1, x2, n, &p);
    if (rc != PL_OK)
        return rc;
    rc = refine_shared_focal(c, &p, to_lm(*opt), nullptr, pose, focal, lm_iterations);
    free_problem(&p);
    return rc;
}
int pl_ransac_relpose(const double *x1, const double *x2, size_t n, const pl_robust_options *opt, pl_camera_pose *pose,
                      uint8_t *inliers, pl_ransac_stats *stats) {
    return ransac_oneshot(EST_REL, x1, x2, n, opt, pose, inliers, stats);
}
int pl_ransac_fundamental(const double *x1, const double *x2, size_t n, const pl_robust_options *opt, double *F,
                          uint8_t *inliers, pl_ransac_stats *stats) {
    return ransac_oneshot(EST_FUND, x1, x2, n, opt, F, inliers, stats);
}
int pl_ransac_homography(const double *x1, const double *x2, size_t n, const pl_robust_options *opt, double *H,
                         uint8_t *inliers, pl_ransac_stats *stats) {
    return ransac_oneshot(EST_HOM, x1, x2, n, opt, H, inliers, stats);
}

// ransac.cc:388-401: no scaling; the mask is get_inliers_1D_radial's (k_mask<EST_RAD1D>)
int pl_ransac_1D_radial_pnp(const double *x, const double *X, size_t n, const pl_robust_options *opt, pl_camera_pose *pose,
                            uint8_t *inliers, pl_ransac_stats *stats) {
    return ransac_oneshot(EST_RAD1D, x, X, n, opt, pose, inliers, stats);
}
int pl_debug_radial1d_chunk(void) { return radial1d_score_chunk(); }
// Diagnostic: the hypothesis generator of a resident problem on its own, wired by wire_batch_step as a batch step wires it, with the
// outputs of every iteration copied back (the header describes the arguments).  Route 0: the single-problem launch (kinds 1 and
// tangent: the staged generator), 1: the single-kernel 5-point generator, 2: the group form over a table of three slots - inactive,
// this problem with all its iterations, this problem with its first ceil(B / 3) iterations - launched with max_B = B.  Records are
// zeroed before the launch, counts and NaN flags set to 0xffffffff: an entry no lane wrote keeps that value.
namespace {
struct DebugGenSet { // the device buffers one slot of the launch writes; `own`: allocated here (slots 0 and 2 of the group form)
    double *models = nullptr;
    uint32_t *num_models = nullptr, *nan_bits = nullptr;
    BatchCtl *ctl = nullptr;
    char *stage = nullptr;
    bool own = false;
    ~DebugGenSet() {
        if (own)
            for (void *q : {(void *)models, (void *)num_models, (void *)nan_bits, (void *)ctl, (void *)stage})
                if (q)
                    (void)hipFree(q);
    }
};
} // namespace
int pl_debug_generate(pl_problem *p, const uint32_t *samples, uint64_t seed, uint64_t pos_base, const uint32_t *positions, size_t num_iters,
                      uint32_t slots_per_iter, int real_focal_check, int route, double *models, uint32_t *num_models, uint32_t *nan_bits,
                      uint32_t *blk_tot, uint32_t *blk_nan, uint32_t *flags) {
    if (!p || !models || !num_models || !blk_tot || !blk_nan || !flags)
        return fail(PL_ERR_INVALID, "null argument");
    if ((samples != nullptr) == (positions != nullptr))
        return fail(PL_ERR_INVALID, "give explicit samples or draw positions, not both");
    const int kind = p->kind;
    if (kind != EST_ABS && kind != EST_REL && kind != EST_FUND && kind != EST_HOM && kind != EST_RELT && kind != EST_RAD1D)
        return fail(PL_ERR_INVALID, "problem kind has no generator");
    if (route < 0 || route > 2 || (route == 1 && kind != EST_REL))
        return fail(PL_ERR_INVALID, "route: 0 single launch, 1 single-kernel generator (kind 1 only), 2 group form");
    if (route == 2 && (kind == EST_RELT || kind == EST_RAD1D))
        return fail(PL_ERR_INVALID, "tangent and 1D-radial problems have no group form");
    if (slots_per_iter < 1 || slots_per_iter > (uint32_t)max_models(kind) || num_iters == 0 || num_iters > (1u << 20))
        return fail(PL_ERR_INVALID, "slots_per_iter must be 1..max_models(kind), num_iters 1..2^20");
    const uint32_t K = (uint32_t)sample_size(kind);
    if (samples) {
        for (size_t i = 0; i < (size_t)K * num_iters; ++i)
            if (samples[i] >= p->n)
                return fail(PL_ERR_INVALID, "sample index beyond the problem's correspondences");
    } else if (p->n < K) {
        return fail(PL_ERR_INVALID, "fewer correspondences than a minimal sample");
    }
    Context *c;
    int rc = get_context(&c);
    if (rc != PL_OK)
        return rc;
    if (p->device != c->device)
        return fail(PL_ERR_INVALID, "problem lives on another device than the calling thread's");
    const uint32_t B = (uint32_t)num_iters, nblk = batch_blocks(B);
    const int members = route == 2 ? 2 : 1;
    BatchRun run{};
    run.kind = kind;
    run.pts = p->ps;
    run.seed = seed, run.pos = pos_base;
    run.real_focal_check = real_focal_check;
    run.explicit_samples = samples != nullptr;
    BatchShape s{};
    s.B = s.Bl = B, s.slots = slots_per_iter, s.chunks = 1;
    s.use_mfma = kind == EST_ABS; // (the scorer that reads the generator's NaN flags: wire_batch_step hands them over only then)
    const BatchSizes z = batch_step_sizes(kind, s);
    BatchBuffers bb;
    rc = context_batch_buffers(c, z, bb);
    if (rc != PL_OK)
        return rc;
    // slot 1 writes the Context's buffers; the group form's slots 2 and 0 get output buffers of their own, of the same size
    DebugGenSet set[3];
    set[0].models = bb.models, set[0].num_models = bb.num_models, set[0].nan_bits = bb.nan_bits, set[0].ctl = bb.ctl, set[0].stage = bb.gen_stage;
    const int nsets = route == 2 ? 3 : 1;
    for (int k = 1; k < nsets; ++k) {
        set[k].own = true;
        HIP_TRY(hipMalloc((void **)&set[k].models, z.models));
        HIP_TRY(hipMalloc((void **)&set[k].num_models, z.num_models));
        if (z.nan_bits)
            HIP_TRY(hipMalloc((void **)&set[k].nan_bits, z.nan_bits));
        HIP_TRY(hipMalloc((void **)&set[k].ctl, z.ctl));
        if (z.gen_stage)
            HIP_TRY(hipMalloc((void **)&set[k].stage, z.gen_stage));
    }
    for (int k = 0; k < nsets; ++k) {
        HIP_TRY(hipMemsetAsync(set[k].models, 0, z.models, c->stream));
        HIP_TRY(hipMemsetAsync(set[k].num_models, 0xff, z.num_models, c->stream));
        if (z.nan_bits)
            HIP_TRY(hipMemsetAsync(set[k].nan_bits, 0xff, z.nan_bits, c->stream));
        HIP_TRY(hipMemsetAsync(set[k].ctl, 0, z.ctl, c->stream));
    }
    if (samples)
        HIP_TRY(hipMemcpyAsync(bb.samples, samples, sizeof(uint32_t) * K * B, hipMemcpyHostToDevice, c->stream));
    else
        HIP_TRY(hipMemcpyAsync(bb.positions, positions, sizeof(uint32_t) * B, hipMemcpyHostToDevice, c->stream));
    // the arguments of slot `k`'s generator over `iters` iterations: the batch step's own wiring on that slot's output buffers
    auto wire = [&](GroupArgs &a, const DebugGenSet &o, uint32_t iters) {
        BatchBuffers b = bb;
        b.models = o.models, b.num_models = o.num_models, b.nan_bits = o.nan_bits, b.ctl = o.ctl, b.gen_stage = o.stage;
        BatchShape sk = s;
        sk.Bl = iters;
        wire_batch_step(a, run, sk, b);
        if (route == 1)
            a.gen.stage = nullptr;
    };
    const uint32_t iters_of[2] = {B, (B + 2) / 3};
    struct Scratch { // freed on every path
        void *p = nullptr;
        ~Scratch() {
            if (p)
                (void)hipFree(p);
        }
    } dtable;
    GroupArgs ha[3];
    if (route == 2) {
        wire(ha[0], set[2], B);
        ha[0].active = 0;
        wire(ha[1], set[0], iters_of[0]);
        wire(ha[2], set[1], iters_of[1]);
        HIP_TRY(hipMalloc(&dtable.p, sizeof(ha)));
        HIP_TRY(hipMemcpyAsync(dtable.p, ha, sizeof(ha), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(launch_group_generate(kind, static_cast<const GroupArgs *>(dtable.p), B, 3, c->stream));
    } else {
        wire(ha[1], set[0], B);
        HIP_TRY(launch_generate(kind, ha[1].gen, c->stream));
    }
    const size_t rec_doubles = (size_t)kModelStride * B * slots_per_iter;
    std::vector<unsigned char> hctl[3];
    for (int k = 0; k < nsets; ++k)
        hctl[k].resize(z.ctl);
    for (int m = 0; m < members; ++m) {
        HIP_TRY(hipMemcpyAsync(models + m * rec_doubles, set[m].models, sizeof(double) * rec_doubles, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(num_models + (size_t)m * B, set[m].num_models, sizeof(uint32_t) * B, hipMemcpyDeviceToHost, c->stream));
        if (nan_bits && z.nan_bits)
            HIP_TRY(hipMemcpyAsync(nan_bits + (size_t)m * B, set[m].nan_bits, sizeof(uint32_t) * B, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(hctl[m].data(), set[m].ctl, z.ctl, hipMemcpyDeviceToHost, c->stream));
    }
    std::vector<double> idle_models;
    std::vector<uint32_t> idle_words;
    if (route == 2) { // what the inactive slot's launch left of its buffers
        idle_models.resize(rec_doubles);
        idle_words.resize(2 * (size_t)B);
        HIP_TRY(hipMemcpyAsync(idle_models.data(), set[2].models, sizeof(double) * rec_doubles, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(idle_words.data(), set[2].num_models, sizeof(uint32_t) * B, hipMemcpyDeviceToHost, c->stream));
        if (z.nan_bits)
            HIP_TRY(hipMemcpyAsync(idle_words.data() + B, set[2].nan_bits, sizeof(uint32_t) * B, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(hctl[2].data(), set[2].ctl, z.ctl, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(wait_stream(c));
    flags[0] = flags[1] = flags[2] = 0;
    for (int m = 0; m < members; ++m) { // the tables behind the control block, laid out for the member's own iterations
        BatchCtl ctl;
        std::memcpy(&ctl, hctl[m].data(), sizeof(ctl));
        flags[m] = ctl.gen_overflow;
        const uint32_t nb = batch_blocks(iters_of[m]);
        const uint32_t *tab = reinterpret_cast<const uint32_t *>(hctl[m].data() + sizeof(BatchCtl));
        for (uint32_t b = 0; b < nblk; ++b) {
            blk_tot[(size_t)m * nblk + b] = b < nb ? tab[b] : 0u;
            blk_nan[(size_t)m * nblk + b] = b < nb ? tab[nb + b] : 0u;
        }
    }
    if (route == 2) {
        uint32_t changed = 0;
        for (double v : idle_models) {
            uint64_t bits;
            std::memcpy(&bits, &v, sizeof(bits));
            changed += bits ? 1u : 0u;
        }
        for (size_t i = 0; i < (z.nan_bits ? 2 : 1) * (size_t)B; ++i)
            changed += idle_words[i] != 0xffffffffu ? 1u : 0u;
        for (unsigned char v : hctl[2])
            changed += v ? 1u : 0u;
        flags[2] = changed;
    }
    return PL_OK;
}
int pl_debug_radial1d_generate(pl_problem *p, const uint32_t *samples, size_t num_iters, uint32_t slots_per_iter, double *models,
                               uint32_t *num_models, uint32_t *totals) {
    if (!p || !samples || !models || !num_models || !totals)
        return fail(PL_ERR_INVALID, "null argument");
    if (p->kind != EST_RAD1D)
        return fail(PL_ERR_INVALID, "not a 1D-radial problem");
    if (num_iters == 0 || num_iters > (1u << 20))
        return fail(PL_ERR_INVALID, "num_iters must be 1..2^20");
    const uint32_t nblk = batch_blocks((uint32_t)num_iters);
    std::vector<uint32_t> tab(2 * (size_t)nblk);
    uint32_t flags[3];
    const int rc = pl_debug_generate(p, samples, 0, 0, nullptr, num_iters, slots_per_iter, 0, 0, models, num_models, nullptr, tab.data(),
                                     tab.data() + nblk, flags);
    if (rc != PL_OK)
        return rc;
    totals[0] = totals[1] = 0;
    for (uint32_t b = 0; b < nblk; ++b)
        totals[0] += tab[b], totals[1] += tab[nblk + b];
    totals[2] = flags[0];
    return PL_OK;
}

// Diagnostic: one stage of the two focal-length estimators on its own (the header describes the arguments).  The argument blocks are
// filled by the group policies' gen_args / score_args / lo_task - the functions driver_focal_group.inc wires its members with, which
// set what DeviceFocalBackend / DeviceSFocalBackend set field by field - and go through the production launchers; nothing here
// selects a kernel.  Where the back ends keep a buffer is where it lives here: models, counts per iteration, the solver workspace and
// the mask in device memory; the mirrors, the scores and the task records in pinned mapped memory.
extern "C++" { // (overloads and a template inside the C interface's block)
namespace {
constexpr unsigned char kStageFillCounter = 0xff, kStageFill = 0x5a;
struct StageBuffers { // one member's buffers, released on every path
    void *dev[4] = {nullptr, nullptr, nullptr, nullptr};   // generate: models, num_models, stage | score: models, num_models | mask: mask
    void *host[4] = {nullptr, nullptr, nullptr, nullptr};  // generate: host_models, host_num_models, positions / samples | score: counts, sums, tasks | mask: host_mask
    void *hdev[4] = {nullptr, nullptr, nullptr, nullptr};  // host[k] as the device addresses it
    ~StageBuffers() {
        for (void *q : dev)
            if (q)
                (void)hipFree(q);
        for (void *q : host)
            if (q)
                (void)hipHostFree(q);
    }
    hipError_t device(int k, size_t bytes) { return hipMalloc(&dev[k], std::max<size_t>(bytes, 256)); }
    hipError_t pinned(int k, size_t bytes) {
        hipError_t e = hipHostMalloc(&host[k], std::max<size_t>(bytes, 256), hipHostMallocMapped);
        return e != hipSuccess ? e : hipHostGetDevicePointer(&hdev[k], host[k], 0);
    }
};
inline hipError_t stage_generate(const FocalGenArgs &g, hipStream_t s) { return launch_focal_generate(g, s); }
inline hipError_t stage_generate(const SFocalGenArgs &g, hipStream_t s) { return launch_sfocal_generate(g, s); }
inline hipError_t stage_score(const FocalScoreArgs &a, hipStream_t s) { return launch_focal_score(a, s); }
inline hipError_t stage_score(const SFocalScoreArgs &a, hipStream_t s) { return launch_sfocal_score(a, s); }
inline hipError_t stage_mask(PnpfGroupPolicy *, const FocalMaskArgs &a, hipStream_t s) {
    return launch_focal_mask(a.a, a.n, a.model, a.thr2, a.mask, a.host_mask, s);
}
inline hipError_t stage_mask(SFocalGroupPolicy *, const FocalMaskArgs &a, hipStream_t s) {
    return launch_sfocal_mask(a.a, a.n, a.model, a.thr2, a.mask, a.host_mask, s);
}

template <class P> int debug_focal_stage(Context *c, int stage, bool group, bool wg, pl_focal_stage_member *ms, uint32_t G) {
    using GenArgs = typename P::GenArgs;
    using ScoreArgs = typename P::ScoreArgs;
    using Task = typename P::Task;
    constexpr uint32_t K = P::Traits::kSample, M = P::Traits::kMaxModels;
    std::vector<StageBuffers> bufs(G);
    std::vector<FocalGroupItem> items(G);
    std::vector<GenArgs> ga(G);
    std::vector<ScoreArgs> sa(G);
    std::vector<FocalMaskArgs> ma(G);
    uint32_t extent_max = 0;
    for (uint32_t k = 0; k < G; ++k) {
        const pl_focal_stage_member &m = ms[k];
        StageBuffers &b = bufs[k];
        FocalGroupItem &g = items[k];
        g.prob = *m.problem;
        g.n = m.idle ? 0u : m.problem->n;
        g.max_focal = m.max_focal;
        g.thr2 = m.thr2;
        g.lm_lo = lo_options(std::sqrt(std::max(m.thr2, 0.0)));
        const uint32_t count = m.idle ? 0u : m.count, cap = m.capacity;
        if (stage == 0) {
            const size_t mod_bytes = sizeof(FocalModel) * (size_t)cap * M, nm_bytes = sizeof(uint32_t) * (size_t)cap;
            HIP_TRY(b.device(0, mod_bytes));
            HIP_TRY(b.device(1, nm_bytes));
            HIP_TRY(b.device(2, P::stage_bytes(std::max(cap, 1u))));
            HIP_TRY(b.pinned(0, mod_bytes));
            HIP_TRY(b.pinned(1, nm_bytes));
            HIP_TRY(b.pinned(2, sizeof(uint32_t) * (size_t)std::max(cap, 1u) * K));
            HIP_TRY(hipMemsetAsync(b.dev[0], kStageFill, mod_bytes, c->stream));
            HIP_TRY(hipMemsetAsync(b.dev[1], kStageFillCounter, nm_bytes, c->stream));
            std::memset(b.host[0], kStageFill, mod_bytes);
            std::memset(b.host[1], kStageFillCounter, nm_bytes);
            // (the generator reads the positions / samples from the pinned block itself, as in the back ends)
            if (count)
                std::memcpy(b.host[2], m.samples ? m.samples : m.positions, sizeof(uint32_t) * (size_t)count * (m.samples ? K : 1));
            GenArgs &a = ga[k];
            P::gen_args(a, g);
            a.n = g.n;
            a.seed = m.seed;
            a.pos_base = m.pos_base;
            a.positions = static_cast<const uint32_t *>(b.hdev[2]);
            a.samples = m.samples ? static_cast<const uint32_t *>(b.hdev[2]) : nullptr;
            a.num_iters = count;
            a.models = static_cast<FocalModel *>(b.dev[0]);
            a.num_models = static_cast<uint32_t *>(b.dev[1]);
            a.stage = static_cast<double *>(b.dev[2]);
            a.explicit_in = nullptr;
            a.host_models = static_cast<FocalModel *>(b.hdev[0]);
            a.host_num_models = static_cast<uint32_t *>(b.hdev[1]);
            extent_max = std::max(extent_max, count);
        } else if (stage == 1) {
            const size_t cnt_bytes = sizeof(uint32_t) * (size_t)cap, sum_bytes = sizeof(double) * (size_t)cap;
            HIP_TRY(b.device(0, sizeof(FocalModel) * (size_t)std::max(count, 1u)));
            HIP_TRY(b.device(1, sizeof(uint32_t) * (size_t)(count / M + 1)));
            HIP_TRY(b.pinned(0, cnt_bytes));
            HIP_TRY(b.pinned(1, sum_bytes));
            HIP_TRY(b.pinned(2, sizeof(Task) * (size_t)std::max(count, 1u)));
            std::memset(b.host[0], kStageFillCounter, cnt_bytes);
            std::memset(b.host[1], kStageFill, sum_bytes);
            const FocalModel *models = reinterpret_cast<const FocalModel *>(m.models);
            if (count && !m.as_tasks)
                HIP_TRY(hipMemcpyAsync(b.dev[0], models, sizeof(FocalModel) * (size_t)count, hipMemcpyHostToDevice, c->stream));
            if (count && m.num_models)
                HIP_TRY(hipMemcpyAsync(b.dev[1], m.num_models, sizeof(uint32_t) * (size_t)(count / M), hipMemcpyHostToDevice, c->stream));
            Task *ht = static_cast<Task *>(b.host[2]);
            for (uint32_t j = 0; m.as_tasks && j < count; ++j) // the record a local optimisation is enqueued with; no refinement runs
                P::lo_task(ht[j], g, models[j], nullptr);
            ScoreArgs &a = sa[k];
            P::score_args(a, g, m.as_tasks ? static_cast<const Task *>(b.hdev[2]) : nullptr, static_cast<uint32_t *>(b.hdev[0]),
                          static_cast<double *>(b.hdev[1]));
            a.models = m.as_tasks ? nullptr : static_cast<const FocalModel *>(b.dev[0]);
            a.num_models = m.num_models ? static_cast<const uint32_t *>(b.dev[1]) : nullptr;
            a.num_slots = count;
            extent_max = std::max(extent_max, count);
        } else {
            HIP_TRY(b.device(0, cap));
            HIP_TRY(b.pinned(0, cap));
            HIP_TRY(hipMemsetAsync(b.dev[0], kStageFill, cap, c->stream));
            std::memset(b.host[0], kStageFill, cap);
            FocalMaskArgs &a = ma[k];
            std::memset(&a, 0, sizeof(a));
            for (int d = 0; d < P::kNd; ++d)
                a.a[d] = g.prob.ps.a[d];
            a.n = g.n;
            std::memcpy(&a.model, m.models, sizeof(FocalModel));
            a.thr2 = m.thr2;
            a.mask = static_cast<uint8_t *>(b.dev[0]);
            a.host_mask = static_cast<uint8_t *>(b.hdev[0]);
            extent_max = std::max(extent_max, g.n);
        }
    }
    struct Table { // freed on every path
        void *p = nullptr;
        ~Table() {
            if (p)
                (void)hipFree(p);
        }
    } table;
    auto upload = [&](const void *src, size_t bytes) -> hipError_t {
        hipError_t e = hipMalloc(&table.p, bytes);
        return e != hipSuccess ? e : hipMemcpyAsync(table.p, src, bytes, hipMemcpyHostToDevice, c->stream);
    };
    if (stage == 0) {
        if (group) {
            HIP_TRY(upload(ga.data(), sizeof(GenArgs) * G));
            HIP_TRY(P::generate(static_cast<const GenArgs *>(table.p), G, extent_max, c->stream));
        } else {
            HIP_TRY(stage_generate(ga[0], c->stream));
        }
    } else if (stage == 1) {
        if (group) {
            HIP_TRY(upload(sa.data(), sizeof(ScoreArgs) * G));
            HIP_TRY(P::score(static_cast<const ScoreArgs *>(table.p), G, extent_max, wg, c->stream));
        } else {
            HIP_TRY(stage_score(sa[0], c->stream));
        }
    } else {
        if (group) {
            HIP_TRY(upload(ma.data(), sizeof(FocalMaskArgs) * G));
            HIP_TRY(P::mask(static_cast<const FocalMaskArgs *>(table.p), G, extent_max, c->stream));
        } else {
            HIP_TRY(stage_mask(static_cast<P *>(nullptr), ma[0], c->stream));
        }
    }
    for (uint32_t k = 0; k < G; ++k) {
        const pl_focal_stage_member &m = ms[k];
        const uint32_t cap = m.capacity;
        if (stage == 0) {
            HIP_TRY(hipMemcpyAsync(m.out_models, bufs[k].dev[0], sizeof(FocalModel) * (size_t)cap * M, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipMemcpyAsync(m.out_num_models, bufs[k].dev[1], sizeof(uint32_t) * (size_t)cap, hipMemcpyDeviceToHost, c->stream));
        } else if (stage == 2) {
            HIP_TRY(hipMemcpyAsync(m.out_mask, bufs[k].dev[0], cap, hipMemcpyDeviceToHost, c->stream));
        }
    }
    HIP_TRY(wait_stream(c));
    for (uint32_t k = 0; k < G; ++k) { // what the kernels wrote into pinned memory themselves
        const pl_focal_stage_member &m = ms[k];
        const uint32_t cap = m.capacity;
        if (stage == 0) {
            std::memcpy(m.out_host_models, bufs[k].host[0], sizeof(FocalModel) * (size_t)cap * M);
            std::memcpy(m.out_host_num_models, bufs[k].host[1], sizeof(uint32_t) * (size_t)cap);
        } else if (stage == 1) {
            std::memcpy(m.out_counts, bufs[k].host[0], sizeof(uint32_t) * (size_t)cap);
            std::memcpy(m.out_sums, bufs[k].host[1], sizeof(double) * (size_t)cap);
        } else {
            std::memcpy(m.out_host_mask, bufs[k].host[0], cap);
        }
    }
    return PL_OK;
}
} // namespace
} // extern "C++"
int pl_debug_focal_stage(int stage, int group, int workgroup_per_model, pl_focal_stage_member *members, size_t num_members) {
    if (!members)
        return fail(PL_ERR_INVALID, "null argument");
    if (stage < 0 || stage > 2 || group < 0 || group > 1)
        return fail(PL_ERR_INVALID, "stage: 0 generate, 1 score, 2 mask; group: 0 single launch, 1 group form");
    if (num_members < 1 || num_members > 8 || (!group && num_members != 1))
        return fail(PL_ERR_INVALID, "one member for the single launch, 1..8 for the group form");
    for (size_t k = 0; k < num_members; ++k)
        if (!members[k].problem)
            return fail(PL_ERR_INVALID, "null argument");
    const int kind = members[0].problem->kind;
    if (kind != EST_ABS && kind != EST_FUND)
        return fail(PL_ERR_INVALID, "the focal-length stages work on problems of kind 0 (absolute pose) or 2 (two views)");
    const uint32_t K = kind == EST_ABS ? kFocalSample : kSFocalSample, M = kind == EST_ABS ? kFocalMaxModels : kSFocalMaxModels;
    for (size_t k = 0; k < num_members; ++k) {
        const pl_focal_stage_member &m = members[k];
        if (m.problem->kind != kind)
            return fail(PL_ERR_INVALID, "the members of one call have the same problem kind");
        const bool outputs = stage == 0   ? m.out_models && m.out_num_models && m.out_host_models && m.out_host_num_models
                             : stage == 1 ? m.out_counts && m.out_sums
                                          : m.out_mask && m.out_host_mask;
        if (!outputs)
            return fail(PL_ERR_INVALID, "null argument");
        if (stage == 2) {
            if (!m.models)
                return fail(PL_ERR_INVALID, "null argument");
            if (m.capacity < m.problem->n || m.capacity == 0)
                return fail(PL_ERR_INVALID, "capacity below the problem's size");
            continue;
        }
        if (m.count > (1u << 20) || (!m.idle && m.count == 0) || m.capacity < m.count || m.capacity == 0)
            return fail(PL_ERR_INVALID, "count must be 1..2^20 (0 for an idle member) and capacity at least count");
        if (m.idle)
            continue;
        if (stage == 0) {
            if ((m.samples != nullptr) == (m.positions != nullptr))
                return fail(PL_ERR_INVALID, "give explicit samples or draw positions, not both");
            if (m.samples) {
                for (size_t i = 0; i < (size_t)K * m.count; ++i)
                    if (m.samples[i] >= m.problem->n)
                        return fail(PL_ERR_INVALID, "sample index beyond the problem's correspondences");
            } else if (m.problem->n < K) {
                return fail(PL_ERR_INVALID, "fewer correspondences than a minimal sample");
            }
        } else {
            if (!m.models)
                return fail(PL_ERR_INVALID, "null argument");
            if (m.num_models && m.count % M != 0)
                return fail(PL_ERR_INVALID, "a gated slot count is a multiple of the models per iteration");
            if (group && !workgroup_per_model && kind == EST_FUND && !m.num_models)
                return fail(PL_ERR_INVALID, "the shared-focal group scorer by iterations needs num_models");
        }
    }
    Context *c;
    int rc = get_context(&c);
    if (rc != PL_OK)
        return rc;
    for (size_t k = 0; k < num_members; ++k)
        if (members[k].problem->device != c->device)
            return fail(PL_ERR_INVALID, "problem lives on another device than the calling thread's");
    if (kind == EST_ABS)
        return debug_focal_stage<PnpfGroupPolicy>(c, stage, group != 0, workgroup_per_model != 0, members, (uint32_t)num_members);
    return debug_focal_stage<SFocalGroupPolicy>(c, stage, group != 0, workgroup_per_model != 0, members, (uint32_t)num_members);
}

// ---------------------------------------------------------------------------- front-ends (robust.cc)
// the final bundle of a front-end over the inliers of the loop's model (the device mask ransac_core / run_focal left in c->mask)
int front_final_refine(Context *c, pl_problem *p, const FrontEnd &fe, double *rec, CameraParams *cam_refined) {
    const FrontBundle fb = front_bundle(fe);
    double out[kModelStride];
    *cam_refined = fb.cam;
    int rc = final_refine(c, p, rec, fb.opt, fb.cam, fb.point_scale, out, nullptr, fb.cam_flags, cam_refined);
    if (rc == PL_OK)
        std::memcpy(rec, out, sizeof(out));
    return rc;
}

// absolute pose behind front_begin: the loop, the gated bundle on the raw pixels, front_finish.  bound: the pre-filter bound when the
// points are already on the device (c->raw_src_*; points2D / points3D are then null), otherwise the host arrays are uploaded
int absolute_pose_run(Context *c, FrontEnd &fe, const double *points2D, const double *points3D, size_t n, const float *bound,
                      const pl_robust_options *opt, pl_camera *camera, pl_camera_pose *pose, uint8_t *inliers, pl_ransac_stats *stats) {
    pl_problem p;
    int rc = make_problem_prepared(c, EST_ABS, points2D, points3D, n, fe.prep, &p, /*resident=*/bound != nullptr, false, bound);
    if (rc != PL_OK)
        return rc;
    pl_ransac_stats local;
    pl_ransac_stats *st = stats ? stats : &local;
    double rec[kModelStride];
    if (opt->estimate_focal_length) { // robust.cc:47-54: ransac_pnpf on the un-projected points, the camera takes its focal length
        double focal = 1.0;
        rc = run_focal(c, &p, &fe.scaled, pose, &focal, inliers, st, points2D, &fe.cam);
        if (rc == PL_OK) {
            front_set_focal(fe, camera, focal);
            record_from_pose(pose, false, rec);
        }
    } else {
        front_initial_record(fe, pose, rec);
        rc = ransac_core(c, &p, &fe.scaled, rec, inliers, st);
    }
    free_problem(&p);
    if (rc != PL_OK)
        return rc;
    if (st->num_inliers <= front_min_inliers(EST_ABS)) {
        front_finish(fe, rec, nullptr, pose, nullptr);
        return PL_OK;
    }
    // the bundle sees the pixels as they are (scaled by 1 / focal: front_bundle)
    CameraParams raw_cam;
    std::memset(&raw_cam, 0, sizeof(raw_cam));
    raw_cam.model_id = CAM_NULL;
    rc = make_problem_prepared(c, EST_ABS, points2D, points3D, n, prepare_unproject(raw_cam, nullptr), &p,
                               /*resident=*/true, /*lm_only=*/true);
    if (rc != PL_OK)
        return rc;
    CameraParams refined;
    rc = front_final_refine(c, &p, fe, rec, &refined);
    free_problem(&p);
    if (rc != PL_OK)
        return rc;
    front_finish(fe, rec, &refined, pose, camera);
    return PL_OK;
}

int pl_estimate_absolute_pose(const double *points2D, const double *points3D, size_t n, const pl_robust_options *opt,
                              pl_camera *camera, pl_camera_pose *pose, uint8_t *inliers, pl_ransac_stats *stats) {
    int rc = validate_options(opt, /*focal_entry=*/true);
    if (rc != PL_OK)
        return rc;
    if (!camera || !camera_supported(camera))
        return fail(PL_ERR_UNSUPPORTED, "camera model not supported (NULL, SIMPLE_PINHOLE, PINHOLE, SIMPLE_RADIAL, RADIAL, OPENCV, OPENCV_FISHEYE, SIMPLE_RADIAL_FISHEYE, RADIAL_FISHEYE)");
    Context *c;
    rc = get_context(&c);
    if (rc != PL_OK)
        return rc;
    FrontEnd fe;
    front_begin(fe, EST_ABS, points2D, points3D, n, *opt, camera, nullptr);
    return absolute_pose_run(c, fe, points2D, points3D, n, nullptr, opt, camera, pose, inliers, stats);
}

// The 1D-radial front-end behind its scale and the block of scaled pixels (the host form below and
// pl_estimate_1D_radial_absolute_pose_dev): max_error and bundle.loss_scale follow the pixels, the loop, the gated bundle; the problem is
// freed
int radial1d_run(Context *c, pl_problem *p, double scale, const pl_robust_options *opt, pl_camera_pose *pose, uint8_t *inliers,
                 pl_ransac_stats *st) {
    pl_robust_options so = *opt;
    so.max_error *= scale;
    so.bundle.loss_scale *= scale;
    double rec[kModelStride];
    if (so.ransac.score_initial_model)
        record_from_pose(pose, false, rec);
    else
        identity_record(EST_RAD1D, rec);
    int rc = ransac_core(c, p, &so, rec, inliers, st);
    if (rc == PL_OK && st->num_inliers > 5) {
        CameraParams none;
        std::memset(&none, 0, sizeof(none));
        none.model_id = CAM_NULL;
        double out[kModelStride];
        rc = final_refine(c, p, rec, to_lm(so.bundle), none, 1.0, out, nullptr);
        if (rc == PL_OK)
            std::memcpy(rec, out, sizeof(out));
    }
    free_problem(p);
    if (rc != PL_OK)
        return rc;
    pose_from_record(rec, pose);
    return PL_OK;
}

// robust.cc:889-934: absolute pose of a 1D-radial camera from centred pixels.  The pixels are multiplied by n / sum |x_k| (summed in
// index order) on the host as they are copied into the problem's block (one pass for the sum, the product in make_problem's copy;
// the block is the resident-problem kind, uploaded once: its cost next to the pinned staging path has not been measured);
// max_error and bundle.loss_scale with them.  The loop is
// ransac_1D_radial_pnp's, the final bundle (bundle_adjust_1D_radial over the inliers, when there are more than 5) takes the caller's
// bundle options; bundle.refine_* has no effect, as in the reference.  n < 5: default stats, pose and inliers untouched.
int pl_estimate_1D_radial_absolute_pose(const double *points2D, const double *points3D, size_t n, const pl_robust_options *opt,
                                        pl_camera_pose *pose, uint8_t *inliers, pl_ransac_stats *stats) {
    int rc = validate_options(opt);
    if (rc != PL_OK)
        return rc;
    if (!pose || ((!points2D || !points3D) && n))
        return fail(PL_ERR_INVALID, "points / pose pointer is null");
    pl_ransac_stats local;
    pl_ransac_stats *st = stats ? stats : &local;
    if (n < 5) {
        std::memset(st, 0, sizeof(*st));
        return PL_OK;
    }
    Context *c;
    rc = get_context(&c);
    if (rc != PL_OK)
        return rc;
    double scale = 0.0;
    for (size_t k = 0; k < n; ++k)
        scale += std::sqrt(0.0 + points2D[2 * k] * points2D[2 * k] + points2D[2 * k + 1] * points2D[2 * k + 1]);
    scale = static_cast<double>(n) / scale;
    pl_problem p;
    rc = make_problem(c, EST_RAD1D, points2D, points3D, n, &p, scale); // (the pixels are multiplied as they are copied)
    if (rc != PL_OK)
        return rc;
    return radial1d_run(c, &p, scale, opt, pose, inliers, st);
}

// relative pose, fundamental matrix, homography: validate, front_begin, the loop, the gated bundle, front_finish
// ... behind front_begin.  bound: as for absolute_pose_run
int two_view_run(Context *c, const FrontEnd &fe, int kind, const double *x1, const double *x2, size_t n, const float *bound, void *model,
                 uint8_t *inliers, pl_ransac_stats *st) {
    double rec[kModelStride];
    front_initial_record(fe, model, rec);
    pl_problem p;
    int rc = make_problem_prepared(c, kind, x1, x2, n, fe.prep, &p, /*resident=*/bound != nullptr, false, bound);
    if (rc != PL_OK)
        return rc;
    rc = ransac_core(c, &p, &fe.scaled, rec, inliers, st);
    if (rc == PL_OK && st->num_inliers > front_min_inliers(kind)) {
        CameraParams refined;
        rc = front_final_refine(c, &p, fe, rec, &refined);
    }
    free_problem(&p);
    if (rc != PL_OK)
        return rc;
    front_finish(fe, rec, nullptr, model, nullptr);
    return PL_OK;
}
int estimate_two_view(int kind, const double *x1, const double *x2, size_t n, const pl_camera *camera1, const pl_camera *camera2,
                      const pl_robust_options *opt, void *model, uint8_t *inliers, pl_ransac_stats *st) {
    Context *c;
    int rc = get_context(&c);
    if (rc != PL_OK)
        return rc;
    FrontEnd fe;
    front_begin(fe, kind, x1, x2, n, *opt, camera1, camera2);
    return two_view_run(c, fe, kind, x1, x2, n, nullptr, model, inliers, st);
}

int pl_estimate_relative_pose(const double *x1, const double *x2, size_t n, const pl_camera *camera1,
                              const pl_camera *camera2, const pl_robust_options *opt, pl_camera_pose *pose,
                              uint8_t *inliers, pl_ransac_stats *stats) {
    // tangent_sampson (robust.cc:255-284) is served here and nowhere else: with fixed cameras, i.e. without bundle.refine_*
    const bool tangent = opt && opt->tangent_sampson;
    pl_robust_options plain;
    if (tangent) {
        plain = *opt;
        plain.tangent_sampson = 0;
    }
    int rc = validate_options(tangent ? &plain : opt);
    if (rc != PL_OK)
        return rc;
    if (tangent && (opt->bundle.refine_focal_length || opt->bundle.refine_principal_point || opt->bundle.refine_extra_params))
        return fail(PL_ERR_UNSUPPORTED, "tangent_sampson with bundle.refine_focal_length / refine_principal_point / refine_extra_params "
                                        "refines the intrinsics with the pose (CameraRelativePoseRefiner): not served, fixed cameras only");
    if (!camera1 || !camera2 || !camera_supported(camera1) || !camera_supported(camera2))
        return fail(PL_ERR_UNSUPPORTED, "camera model not supported (NULL, SIMPLE_PINHOLE, PINHOLE, SIMPLE_RADIAL, RADIAL, OPENCV, OPENCV_FISHEYE, SIMPLE_RADIAL_FISHEYE, RADIAL_FISHEYE)");
    pl_ransac_stats local;
    return estimate_two_view(tangent ? EST_RELT : EST_REL, x1, x2, n, camera1, camera2, opt, pose, inliers, stats ? stats : &local);
}

// The shared-focal front-end behind its normalisation (robust.cc:386-421; the host form below and
// pl_estimate_shared_focal_relative_pose_dev, whose rows are already on the device: resident, x1 / x2 null)
int shared_focal_run(Context *c, const double *x1, const double *x2, size_t n, const PrepareArgs &prep, double scale, bool resident,
                     const pl_robust_options *opt, pl_camera_pose *pose, double *focal, uint8_t *inliers, pl_ransac_stats *st) {
    pl_robust_options scaled = *opt;
    scaled.max_error /= scale;
    scaled.bundle.loss_scale /= scale;
    double f = *focal;
    if (opt->ransac.score_initial_model) // :392-397
        f = f / scale;
    pl_problem p;
    int rc = make_problem_prepared(c, EST_FUND, x1, x2, n, prep, &p, resident, /*lm_only=*/true);
    if (rc != PL_OK)
        return rc;
    rc = run_shared_focal(c, &p, &scaled, pose, &f, inliers, st);
    if (rc == PL_OK && st->num_inliers > front_min_inliers(kFrontSharedFocal)) // :401-415: refine_shared_focal_relpose over the inliers (c->mask: the device mask)
        rc = refine_shared_focal(c, &p, to_lm(scaled.bundle), c->mask.as<uint8_t>(), pose, &f, nullptr);
    free_problem(&p);
    if (rc != PL_OK)
        return rc;
    *focal = f * scale; // :417 (the caller's cameras: SIMPLE_PINHOLE {focal, pp[0], pp[1]}, :418-421)
    return PL_OK;
}

int pl_estimate_shared_focal_relative_pose(const double *x1, const double *x2, size_t n, const double *pp, const pl_robust_options *opt,
                                           pl_camera_pose *pose, double *focal, uint8_t *inliers, pl_ransac_stats *stats) {
    if (!pp || !pose || !focal)
        return fail(PL_ERR_INVALID, "null argument");
    int rc = validate_options(opt);
    if (rc != PL_OK)
        return rc;
    Context *c;
    rc = get_context(&c);
    if (rc != PL_OK)
        return rc;
    pl_ransac_stats local;
    pl_ransac_stats *st = stats ? stats : &local;
    // robust.cc:373-390
    PrepareArgs prep;
    const double scale = normalization_about(x1, x2, n, pp[0], pp[1], prep);
    return shared_focal_run(c, x1, x2, n, prep, scale, /*resident=*/false, opt, pose, focal, inliers, st);
}

int pl_estimate_fundamental(const double *x1, const double *x2, size_t n, const pl_robust_options *opt, double *F,
                            uint8_t *inliers, pl_ransac_stats *stats) {
    int rc = validate_options(opt);
    if (rc != PL_OK)
        return rc;
    pl_ransac_stats local;
    pl_ransac_stats *st = stats ? stats : &local;
    if (n < 7) { // robust.cc:548-550
        std::memset(st, 0, sizeof(*st));
        st->model_score = std::numeric_limits<double>::max();
        return PL_OK;
    }
    return estimate_two_view(EST_FUND, x1, x2, n, nullptr, nullptr, opt, F, inliers, st);
}

int pl_estimate_homography(const double *x1, const double *x2, size_t n, const pl_robust_options *opt, double *H,
                           uint8_t *inliers, pl_ransac_stats *stats) {
    int rc = validate_options(opt);
    if (rc != PL_OK)
        return rc;
    pl_ransac_stats local;
    pl_ransac_stats *st = stats ? stats : &local;
    if (n < 4) { // robust.cc:716-718
        std::memset(st, 0, sizeof(*st));
        st->model_score = std::numeric_limits<double>::max();
        return PL_OK;
    }
    return estimate_two_view(EST_HOM, x1, x2, n, nullptr, nullptr, opt, H, inliers, st);
}

#include "driver_dev.inc"
#include "driver_scored.inc"

// ---------------------------------------------------------------------------- un-distortion stage
int pl_undistort_points(const pl_camera *camera, const double *points2D, size_t n, double *out) {
    if (undistort_camera_check(camera) != PL_OK) // (driver_dev.inc: the device-memory form says the same)
        return PL_ERR_UNSUPPORTED;
    if (n > 0x7fffffffu)
        return fail(PL_ERR_INVALID, "too many points");
    if (n && (!points2D || !out))
        return fail(PL_ERR_INVALID, "points pointer is null");
    Context *c;
    int rc = get_context(&c);
    if (rc != PL_OK)
        return rc;
    if (n == 0)
        return PL_OK;
    const CameraParams cam = to_cam(camera);
    double fx, fy, cx, cy;
    if (!camera_has_two_focals(camera->model_id))
        fx = fy = cam.p[0], cx = cam.p[1], cy = cam.p[2];
    else
        fx = cam.p[0], fy = cam.p[1], cx = cam.p[2], cy = cam.p[3];
    HIP_TRY(c->raw_a.ensure(sizeof(double) * 2 * n));
    HIP_TRY(c->raw_b.ensure(sizeof(double) * 2 * n));
    HIP_TRY(hipMemcpyAsync(c->raw_a.p, points2D, sizeof(double) * 2 * n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(launch_undistort(c->raw_a.as<double>(), (uint32_t)n, cam, fx, fy, cx, cy, c->raw_b.as<double>(), c->stream));
    HIP_TRY(hipMemcpyAsync(out, c->raw_b.p, sizeof(double) * 2 * n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(wait_stream(c));
    return PL_OK;
}

// ---------------------------------------------------------------------------- minimal solvers
int pl_solve_batch(int kind, const double *in, size_t count, double *out_models, uint32_t *out_counts) {
    if ((kind < 0 || kind > 3) && kind != EST_RAD1D) // (5: p5lp_radial - in: x 5 x 3 (third component not read), X 5 x 3; <= 4 models)
        return fail(PL_ERR_INVALID, "unknown solver kind");
    Context *c;
    int rc = get_context(&c);
    if (rc != PL_OK)
        return rc;
    if (count == 0)
        return PL_OK;
    const int K = sample_size(kind), MAXM = max_models(kind);
    const size_t in_bytes = sizeof(double) * 6 * K * count;
    const size_t out_bytes = sizeof(double) * kModelStride * MAXM * count;
    HIP_TRY(c->solve_in.ensure(in_bytes));
    HIP_TRY(c->solve_out.ensure(out_bytes));
    HIP_TRY(c->solve_cnt.ensure(sizeof(uint32_t) * count));
    HIP_TRY(hipMemcpyAsync(c->solve_in.p, in, in_bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(launch_solve_batch(kind, c->solve_in.as<double>(), (uint32_t)count, c->solve_out.as<double>(),
                               c->solve_cnt.as<uint32_t>(), c->stream));
    HIP_TRY(hipMemcpyAsync(out_models, c->solve_out.p, out_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(out_counts, c->solve_cnt.p, sizeof(uint32_t) * count, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(wait_stream(c));
    return PL_OK;
}

// the two focal-length solvers: kind 0 P3.5Pf (in: x 4 x 2, X 4 x 3 per problem; <= 10 models), kind 1 the 6-point shared-focal
// solver (in: x1 6 x 3, x2 6 x 3 unit bearings per problem; <= 60 models); out_models: 8 doubles (q, t, focal) per slot
int pl_solve_focal_batch(int kind, const double *in, size_t count, double *out_models, uint32_t *out_counts) {
    if (kind < 0 || kind > 1)
        return fail(PL_ERR_INVALID, "unknown focal solver kind");
    if ((!in || !out_models || !out_counts) && count)
        return fail(PL_ERR_INVALID, "null argument");
    Context *c;
    int rc = get_context(&c);
    if (rc != PL_OK)
        return rc;
    if (count == 0)
        return PL_OK;
    if (count > 0x7fffffffu / 64u)
        return fail(PL_ERR_INVALID, "too many problems");
    const size_t per_in = kind == 0 ? 20 : 36, slots = kind == 0 ? (size_t)kFocalMaxModels : (size_t)kSFocalMaxModels;
    const size_t in_bytes = sizeof(double) * per_in * count, out_bytes = sizeof(FocalModel) * slots * count;
    HIP_TRY(c->solve_in.ensure(in_bytes));
    HIP_TRY(c->solve_out.ensure(out_bytes));
    HIP_TRY(c->solve_cnt.ensure(sizeof(uint32_t) * count));
    HIP_TRY(hipMemcpyAsync(c->solve_in.p, in, in_bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(c->solve_out.p, 0, out_bytes, c->stream));
    if (kind == 0) {
        const uint32_t per_pass = (uint32_t)std::min<size_t>(count, 8192);
        HIP_TRY(c->focal_stage.ensure(focal_stage_bytes(per_pass)));
        HIP_TRY(launch_focal_solve(c->solve_in.as<double>(), (uint32_t)count, c->solve_out.as<FocalModel>(), c->solve_cnt.as<uint32_t>(),
                                   c->focal_stage.as<double>(), per_pass, c->stream));
    }
    else {
        const uint32_t per_pass = (uint32_t)std::min<size_t>(count, 8192);
        HIP_TRY(c->focal_stage.ensure(sfocal_stage_bytes(per_pass)));
        HIP_TRY(launch_sfocal_solve(c->solve_in.as<double>(), (uint32_t)count, c->solve_out.as<FocalModel>(), c->solve_cnt.as<uint32_t>(),
                                    c->focal_stage.as<double>(), per_pass, c->stream));
    }
    HIP_TRY(hipMemcpyAsync(out_models, c->solve_out.p, out_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(out_counts, c->solve_cnt.p, sizeof(uint32_t) * count, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(wait_stream(c));
    return PL_OK;
}
static int focal_solve_one(int kind, const double *a, size_t na, const double *b, size_t nb, pl_camera_pose *out, double *focals) {
    if (!a || !b || !out || !focals)
        return fail(PL_ERR_INVALID, "null argument");
    std::vector<double> in(na + nb);
    std::memcpy(in.data(), a, sizeof(double) * na);
    std::memcpy(in.data() + na, b, sizeof(double) * nb);
    const size_t slots = kind == 0 ? (size_t)kFocalMaxModels : (size_t)kSFocalMaxModels;
    std::vector<double> models(8 * slots);
    uint32_t n = 0;
    int rc = pl_solve_focal_batch(kind, in.data(), 1, models.data(), &n);
    if (rc != PL_OK)
        return rc;
    for (uint32_t i = 0; i < n; ++i) {
        for (int k = 0; k < 4; ++k)
            out[i].q[k] = models[8 * i + k];
        for (int k = 0; k < 3; ++k)
            out[i].t[k] = models[8 * i + 4 + k];
        focals[i] = models[8 * i + 7];
    }
    return (int)n;
}
int pl_p35pf(const double *x, const double *X, pl_camera_pose *out, double *focals) { return focal_solve_one(0, x, 8, X, 12, out, focals); }
int pl_relpose_6pt_shared_focal(const double *x1, const double *x2, pl_camera_pose *out, double *focals) {
    return focal_solve_one(1, x1, 18, x2, 18, out, focals);
}

static int solve_one(int kind, const double *a, const double *b, double *records, uint32_t *cnt) {
    const int K = sample_size(kind);
    std::vector<double> in(6 * K);
    std::memcpy(in.data(), a, sizeof(double) * 3 * K);
    std::memcpy(in.data() + 3 * K, b, sizeof(double) * 3 * K);
    return pl_solve_batch(kind, in.data(), 1, records, cnt);
}
int pl_p3p(const double *x, const double *X, pl_camera_pose *out) {
    double rec[4 * kModelStride];
    uint32_t n = 0;
    int rc = solve_one(EST_ABS, x, X, rec, &n);
    if (rc != PL_OK)
        return rc;
    for (uint32_t i = 0; i < n; ++i)
        pose_from_record(rec + i * kModelStride, out + i);
    return (int)n;
}
int pl_p5lp_radial(const double *x, const double *X, pl_camera_pose *out, int *count) {
    if (!x || !X || !out)
        return fail(PL_ERR_INVALID, "null argument");
    double x3[15];
    for (int k = 0; k < 5; ++k)
        x3[3 * k] = x[2 * k], x3[3 * k + 1] = x[2 * k + 1], x3[3 * k + 2] = 0.0;
    double rec[4 * kModelStride];
    uint32_t n = 0;
    int rc = solve_one(EST_RAD1D, x3, X, rec, &n);
    if (rc != PL_OK)
        return rc;
    for (uint32_t i = 0; i < n; ++i)
        pose_from_record(rec + i * kModelStride, out + i);
    if (count)
        *count = (int)n;
    return (int)n;
}
int pl_relpose_5pt(const double *x1, const double *x2, pl_camera_pose *out) {
    std::vector<double> rec(40 * kModelStride);
    uint32_t n = 0;
    int rc = solve_one(EST_REL, x1, x2, rec.data(), &n);
    if (rc != PL_OK)
        return rc;
    for (uint32_t i = 0; i < n; ++i)
        pose_from_record(rec.data() + i * kModelStride, out + i);
    return (int)n;
}
int pl_essential_matrix_5pt(const double *x1, const double *x2, double *E) {
    // kind 4 (internal): essential matrices before the motion decomposition
    Context *c;
    int rc = get_context(&c);
    if (rc != PL_OK)
        return rc;
    std::vector<double> in(30), rec(10 * kModelStride);
    std::memcpy(in.data(), x1, sizeof(double) * 15);
    std::memcpy(in.data() + 15, x2, sizeof(double) * 15);
    uint32_t n = 0;
    HIP_TRY(c->solve_in.ensure(sizeof(double) * 30));
    HIP_TRY(c->solve_out.ensure(sizeof(double) * kModelStride * 10));
    HIP_TRY(c->solve_cnt.ensure(sizeof(uint32_t)));
    HIP_TRY(hipMemcpyAsync(c->solve_in.p, in.data(), sizeof(double) * 30, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(launch_solve_batch(4, c->solve_in.as<double>(), 1, c->solve_out.as<double>(), c->solve_cnt.as<uint32_t>(),
                               c->stream));
    HIP_TRY(hipMemcpyAsync(rec.data(), c->solve_out.p, sizeof(double) * kModelStride * 10, hipMemcpyDeviceToHost,
                           c->stream));
    HIP_TRY(hipMemcpyAsync(&n, c->solve_cnt.p, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(wait_stream(c));
    for (uint32_t i = 0; i < n; ++i) {
        Mat3 M;
        for (int k = 0; k < 9; ++k)
            M.m[k] = rec[i * kModelStride + kMatOff + k];
        mat_to_colmajor(M, E + 9 * i);
    }
    return (int)n;
}
int pl_relpose_7pt(const double *x1, const double *x2, double *F) {
    double rec[3 * kModelStride];
    uint32_t n = 0;
    int rc = solve_one(EST_FUND, x1, x2, rec, &n);
    if (rc != PL_OK)
        return rc;
    for (uint32_t i = 0; i < n; ++i) {
        Mat3 M;
        for (int k = 0; k < 9; ++k)
            M.m[k] = rec[i * kModelStride + kMatOff + k];
        mat_to_colmajor(M, F + 9 * i);
    }
    return (int)n;
}
int pl_homography_4pt(const double *x1, const double *x2, double *H) {
    double rec[kModelStride];
    uint32_t n = 0;
    int rc = solve_one(EST_HOM, x1, x2, rec, &n);
    if (rc != PL_OK)
        return rc;
    if (n) {
        Mat3 M;
        for (int k = 0; k < 9; ++k)
            M.m[k] = rec[kMatOff + k];
        mat_to_colmajor(M, H);
    }
    return (int)n;
}

#include "driver_batch.inc"

} // extern "C"
