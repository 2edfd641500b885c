// poselib_amd - groups of focal-length problems through ONE launch sequence (included by driver.cc, inside its anonymous namespace).
//
// robust.cc:47-54 (estimate_absolute_pose with opt.estimate_focal_length: ransac_pnpf, then the bundle with the focal length free)
// and robust.cc:366-424 (estimate_shared_focal_relative_pose) as citizens of pl_estimate_batch.  Up to round 4 every such item was a
// chain of ~11 dispatches and ~8 synchronisations on its own stream (driver_focal.inc, driver_sfocal.inc): 16 hardware queues bounded
// the throughput at 5.4 k / 4.2 k problems per second.  Here up to kFocalGroupMax problems of one estimator advance in lock-step:
//
//   stage A  front-end arithmetic per item on the host (front_begin, like the single-problem entry points), the raw
//            correspondences of all members -> one pinned block -> one upload; k_prepare_g (un-projection / normalisation)
//            (pl_estimate_shared_focal_relative_pose_batch_dev, members in the caller's device memory: no host pass and no upload of
//            points - k_ingest_g, k_point_stats_g about the members' principal points, then k_prepare_g with the scale read from
//            the member's record on the device; the host reads the records after the stage's one synchronisation)
//   rounds   every member's loop (pl_focal.h FocalLoop - the code the single-problem path runs) is advanced to its next request;
//            the requests of all members are evaluated together - a batch of iterations for the members that ask for one
//            (k_*_setup_g + k_*_solve_g + k_*_score_g, blockIdx.y = member), the local optimisations of the others as ONE launch over
//            all their tasks (k_lm_cam / k_sfocal_lm: a task carries its own correspondences) followed by k_*_score_wg_g on the models
//            the tasks hold - one table upload and ONE synchronisation per round
//   tail     get_inliers of every member's model (k_*_mask_g), the front-ends' final bundles as one launch, one synchronisation
//
// A member's results are those of the single-problem entry point bit for bit (same kernel bodies, same loop code, a result does not
// depend on the group): tests/test_zz_gpu_focal_group.py.  Items the path does not cover (PROSAC, warm starts, the NULL camera, fewer points
// than sample + 4, long fixed-length runs) stay on the single-problem path.

constexpr uint32_t kFocalGroupMax = 64;  // members per launch sequence (pnpf: 8.8 KB of solver workspace per iteration and member)
constexpr uint32_t kSFocalGroupMax = 32; // (shared focal: 60 model slots per iteration are mirrored in pinned memory, 3.8 KB per iteration)

struct DeviceBatch; // (driver_batch.inc)
struct FocalGroupItem {
    pl_batch_item *item = nullptr;
    // pl_estimate_shared_focal_relative_pose_batch_dev (est 1): the member's rows in the caller's device memory - or, for a scored
    // member, the contiguous fp64 blocks its ranking left - and, optionally, where its mask goes there.  dev / index: the call and
    // the item's place in it (a member its group hands back runs through the single _dev entry point)
    const pl_device_points *src_a = nullptr, *src_b = nullptr;
    const MaskDest *mdest = nullptr;
    const DeviceBatch *dev = nullptr;
    size_t index = 0;
    const double *raw_a = nullptr, *raw_b = nullptr; // ... the fp64 AoS blocks k_prepare_g reads (stage A)
    const PointStatsRecord *d_rec = nullptr, *h_rec = nullptr; // ... the member's record of k_point_stats_g: device address, host address
    int est = 0; // 0: absolute pose with unknown focal length, 1: shared-focal relative pose
    uint32_t n = 0;
    bool fallback = false;
    FrontEnd fe;            // front-end (stage A; est 1: scaled, scale and prep of robust.cc:373-390)
    CameraParams cam{};     // est 0: the caller's camera as it came in (snapshot taken when the item is created)
    bool cam_saved = false; // cam holds the caller's camera: a failed group may restore it before the item is retried on its own
    double max_focal = -1.0; // est 0: compute_max_focal_length (absolute_pose.cc:159-177)
    pl_ransac_stats local_st;
    pl_ransac_stats *st = nullptr;
    pl_problem prob;     // the prepared correspondences (borrowed SoA block in the group's arena)
    pl_problem prob_raw; // est 0: the raw pixels next to the 3-D points (the final bundle's problem, robust.cc:103-123)
    uint8_t *d_mask = nullptr;
    size_t raw_a_off = 0, raw_b_off = 0;
    // the loop
    FocalLoopOptions lo;
    LMOptions lm_lo;
    double thr2 = 0.0;
    FocalModel best;
    FocalLoopStats fs;
    int request = 0;
    uint32_t task0 = 0, ntasks = 0; // the member's tasks in the round's LM launch
    double t_start = 0.0;
};

struct FocalGroupContext { // per host thread AND device, kept for later groups
    int device = -1;
    DevBuf pts, raw, args, models, num_models, stage, lm_scratch;
    HostBuf h_raw, h_args, h_pos, h_smp, h_out, h_rout, h_tasks, h_mask; // (h_smp: the PROSAC members' explicit samples of a round)
    HostBuf h_dev_tab; // members in device memory: the tables of k_ingest_g / k_point_stats_g and the members' records
    void release() {
        for (DevBuf *b : {&pts, &raw, &args, &models, &num_models, &stage, &lm_scratch}) {
            if (b->p)
                (void)hipFree(b->p);
            b->p = nullptr, b->cap = 0;
        }
        for (HostBuf *b : {&h_raw, &h_args, &h_pos, &h_smp, &h_out, &h_rout, &h_tasks, &h_mask, &h_dev_tab}) {
            if (b->p)
                (void)hipHostFree(b->p);
            b->p = b->dp = nullptr, b->cap = 0;
        }
    }
};
thread_local FocalGroupContext *g_focal_group_ctx = nullptr;

// which focal estimator a batch item is, -1: none the group path covers (dev: the host-side copy of an item whose points are in
// device memory - a == b == null)
int focal_group_estimator(const pl_batch_item &it, bool dev = false) {
    if (!it.opt || !it.model || !it.camera1 || (!dev && (!it.a || !it.b)))
        return -1;
    const pl_robust_options &o = *it.opt;
    if (o.ransac.score_initial_model)
        return -1; // (warm starts: the single-problem path; PROSAC - samples drawn by the member's loop on the host - is a member since round 6)
    if (o.ransac.max_iterations == 0 || o.ransac.min_iterations > 4096 || it.n > kGroupMaxPoints)
        return -1;
    if (it.kind == EST_ABS && o.estimate_focal_length) {
        if (o.min_fov != o.min_fov || o.tangent_sampson || o.estimate_extra_params)
            return -1; // (validate_options reports these)
        if (!camera_supported(it.camera1) || it.camera1->model_id == CAM_NULL)
            return -1; // (every supported model but NULL: every model whose focal length the estimate can be written to)
        return it.n >= (size_t)kFocalSample + 4 ? 0 : -1;
    }
    if (it.kind == 4) {
        if (o.min_fov != o.min_fov || o.tangent_sampson || o.estimate_focal_length || o.estimate_extra_params)
            return -1;
        if (it.camera1->model_id != CAM_SIMPLE_PINHOLE || it.camera1->num_params < 3)
            return -1;
        return it.n >= (size_t)kSFocalSample + 4 ? 1 : -1;
    }
    return -1;
}

// ---- the two estimators' kernels and argument blocks behind one face ----
struct PnpfGroupPolicy {
    using Traits = PnpfTraits;
    using GenArgs = FocalGenArgs;
    using ScoreArgs = FocalScoreArgs;
    using Task = LMTask;
    static constexpr int kEst = 0, kNd = 5, kDb = 3, kKind = EST_ABS;
    static size_t stage_bytes(uint32_t B) { return focal_stage_bytes(B); }
    static hipError_t generate(const GenArgs *a, uint32_t G, uint32_t max_B, hipStream_t s) { return launch_focal_generate_g(a, G, max_B, s); }
    static hipError_t score(const ScoreArgs *a, uint32_t G, uint32_t max_slots, bool wg, hipStream_t s) { return launch_focal_score_g(a, G, max_slots, wg, s); }
    static hipError_t lm(Task *t, uint32_t count, hipStream_t s) { return launch_lm_cam(t, count, s); }
    static hipError_t mask(const FocalMaskArgs *a, uint32_t G, uint32_t max_n, hipStream_t s) { return launch_focal_mask_g(a, G, max_n, s); }
    static void gen_args(GenArgs &ga, const FocalGroupItem &g) {
        std::memset(&ga, 0, sizeof(ga));
        for (int i = 0; i < kNd; ++i)
            ga.a[i] = g.prob.ps.a[i];
        ga.max_focal = g.max_focal;
    }
    static void score_args(ScoreArgs &sa, const FocalGroupItem &g, const Task *tasks, uint32_t *counts, double *sums) {
        std::memset(&sa, 0, sizeof(sa));
        for (int i = 0; i < kNd; ++i)
            sa.a[i] = g.prob.ps.a[i];
        sa.n = g.n;
        sa.thr2 = g.thr2;
        sa.lm_tasks = tasks;
        sa.counts = counts;
        sa.sums = sums;
    }
    // refine_model (absolute_pose.cc:145-157): pose and focal length on all correspondences, truncated loss
    static void lo_task(Task &t, const FocalGroupItem &g, const FocalModel &seed, uint8_t *) {
        std::memset(&t, 0, sizeof(t));
        t.pts = g.prob.ps;
        for (int i = 0; i < 4; ++i)
            t.params[i] = seed.q[i];
        for (int i = 0; i < 3; ++i)
            t.params[4 + i] = seed.t[i];
        t.opt = g.lm_lo;
        t.cam.model_id = CAM_SIMPLE_PINHOLE;
        t.cam.num_params = 3;
        t.cam.p[0] = seed.f; // {f, 0, 0}
        t.point_scale = 1.0;
        t.cam_flags = CAM_REFINE_FOCAL;
    }
    static bool lo_needs_scratch() { return false; }
    static void lo_result(const Task &t, const FocalModel &, FocalModel &out) {
        for (int i = 0; i < 4; ++i)
            out.q[i] = t.params[i];
        for (int i = 0; i < 3; ++i)
            out.t[i] = t.params[4 + i];
        out.f = t.cam.p[0];
    }
};
struct SFocalGroupPolicy {
    using Traits = SharedFocalTraits;
    using GenArgs = SFocalGenArgs;
    using ScoreArgs = SFocalScoreArgs;
    using Task = SFocalLMTask;
    static constexpr int kEst = 1, kNd = 4, kDb = 2, kKind = EST_FUND;
    static size_t stage_bytes(uint32_t B) { return sfocal_stage_bytes(B); }
    static hipError_t generate(const GenArgs *a, uint32_t G, uint32_t max_B, hipStream_t s) { return launch_sfocal_generate_g(a, G, max_B, s); }
    static hipError_t score(const ScoreArgs *a, uint32_t G, uint32_t max_slots, bool wg, hipStream_t s) { return launch_sfocal_score_g(a, G, max_slots, wg, s); }
    static hipError_t lm(Task *t, uint32_t count, hipStream_t s) { return launch_sfocal_lm(t, count, s); }
    static hipError_t mask(const FocalMaskArgs *a, uint32_t G, uint32_t max_n, hipStream_t s) { return launch_sfocal_mask_g(a, G, max_n, s); }
    static void gen_args(GenArgs &ga, const FocalGroupItem &g) {
        std::memset(&ga, 0, sizeof(ga));
        for (int i = 0; i < kNd; ++i)
            ga.a[i] = g.prob.ps.a[i];
    }
    static void score_args(ScoreArgs &sa, const FocalGroupItem &g, const Task *tasks, uint32_t *counts, double *sums) {
        std::memset(&sa, 0, sizeof(sa));
        for (int i = 0; i < kNd; ++i)
            sa.a[i] = g.prob.ps.a[i];
        sa.n = g.n;
        sa.thr2 = g.thr2;
        sa.lm_tasks = tasks;
        sa.counts = counts;
        sa.scores = sums;
    }
    // refine_model (relative_pose.cc:173-203): the correspondences below 5 thr^2, nothing when <= 6 of them
    static void lo_task(Task &t, const FocalGroupItem &g, const FocalModel &seed, uint8_t *scratch) {
        std::memset(&t, 0, sizeof(t));
        for (int i = 0; i < kNd; ++i)
            t.a[i] = g.prob.ps.a[i];
        t.n = g.n;
        for (int i = 0; i < 4; ++i)
            t.params[i] = seed.q[i];
        for (int i = 0; i < 3; ++i)
            t.params[4 + i] = seed.t[i];
        t.params[kSFocalFocalSlot] = seed.f;
        t.opt = g.lm_lo;
        t.prefilter_thr2 = 5 * g.thr2;
        t.mask = nullptr;
        t.scratch = scratch;
    }
    static bool lo_needs_scratch() { return true; }
    static void lo_result(const Task &t, const FocalModel &seed, FocalModel &out) {
        out = seed;
        if (t.skipped)
            return;
        for (int i = 0; i < 4; ++i)
            out.q[i] = t.params[i];
        for (int i = 0; i < 3; ++i)
            out.t[i] = t.params[4 + i];
        out.f = t.params[kSFocalFocalSlot];
    }
};

// the loop's options and its start from the front-end's scaled options
void focal_group_loop_setup(FocalGroupItem &g) {
    g.lo = focal_loop_options(g.fe.scaled, g.max_focal); // (no warm starts among the members: score_initial_model is 0)
    g.thr2 = g.fe.scaled.max_error * g.fe.scaled.max_error;
    g.lm_lo = lo_options(g.fe.scaled.max_error);
    std::memset(&g.best, 0, sizeof(g.best)); // ransac.cc:61-66 / 185-190
    g.best.q[0] = 1.0;
    g.best.f = 1.0;
}
// stage A, host half: what pl_estimate_absolute_pose / pl_estimate_shared_focal_relative_pose compute before the loop
void focal_group_prepare_item(FocalGroupItem &g) {
    pl_batch_item &it = *g.item;
    g.n = (uint32_t)it.n;
    g.st = it.stats ? it.stats : &g.local_st;
    FrontEnd &fe = g.fe;
    if (g.est == 0) { // robust.cc:40-54
        front_begin(fe, EST_ABS, it.a, it.b, it.n, *it.opt, it.camera1, nullptr);
        g.max_focal = compute_max_focal_length(it.a, it.n, &fe.cam, fe.scaled.min_fov);
    } else { // robust.cc:373-390
        fe = FrontEnd();
        fe.kind = kFrontSharedFocal;
        fe.scaled = *it.opt;
        const double *pp = it.camera1->params + 1;
        fe.scale = normalization_about(it.a, it.b, it.n, pp[0], pp[1], fe.prep);
        fe.scaled.max_error /= fe.scale;
        fe.scaled.bundle.loss_scale /= fe.scale;
        g.max_focal = -1.0;
    }
    focal_group_loop_setup(g);
}
// ... of a shared-focal member whose rows are in device memory: everything but the scale in front of stage A's launches (the
// prepare entry takes the scale from the member's record on the device), the rest - focal_group_prepare_item's code, with the
// reduction's result in place of normalization_about's - once the record is back
void focal_group_begin_device_item(FocalGroupItem &g) {
    pl_batch_item &it = *g.item;
    g.n = (uint32_t)it.n;
    g.st = it.stats ? it.stats : &g.local_st;
    g.fe = FrontEnd();
    g.fe.kind = kFrontSharedFocal;
    g.fe.scaled = *it.opt;
    const double *pp = it.camera1->params + 1;
    prepare_about(pp[0], pp[1], 0.0, g.fe.prep);
    g.max_focal = -1.0;
}
void focal_group_scale_from_device(FocalGroupItem &g) {
    FrontEnd &fe = g.fe;
    fe.scale = fe.prep.scale = g.h_rec->scale;
    fe.scaled.max_error /= fe.scale;
    fe.scaled.bundle.loss_scale /= fe.scale;
    focal_group_loop_setup(g);
}
// k_ingest_g and k_point_stats_g (about the members' principal points) of a group of such members, enqueued on the context's
// stream; sets the members' raw_a / raw_b / d_rec / h_rec (driver_scored.inc)
int focal_group_stage_device(Context *c, FocalGroupContext &gc, FocalGroupItem *const *pit, uint32_t count);

// ---- the tail of the two front-ends: the loop's result into the caller's records, the final bundle's task, its result ----
void focal_group_loop_result(FocalGroupItem &g) {
    pl_camera_pose *pose = static_cast<pl_camera_pose *>(g.item->model);
    for (int i = 0; i < 4; ++i)
        pose->q[i] = g.best.q[i];
    for (int i = 0; i < 3; ++i)
        pose->t[i] = g.best.t[i];
    if (g.est == 0)
        front_set_focal(g.fe, g.item->camera1, g.best.f); // robust.cc:52 (the camera takes the focal length)
}
// robust.cc:103-123 with bundle.refine_focal_length forced (:53): the inliers in focal-normalised pixels, pose and focal length free
void focal_group_bundle_task(LMTask &t, FocalGroupItem &g) {
    const FrontBundle fb = front_bundle(g.fe); // (cam_flags never 0: every model the path takes has a focal length)
    double rec[kModelStride];
    record_from_pose(static_cast<const pl_camera_pose *>(g.item->model), false, rec);
    std::memset(&t, 0, sizeof(t));
    t.pts = g.prob_raw.ps;
    lm_params_from_record(EST_ABS, rec, t.params);
    t.opt = fb.opt;
    t.cam = fb.cam;
    t.point_scale = fb.point_scale;
    t.cam_flags = fb.cam_flags;
    t.mask = g.d_mask;
}
void focal_group_finish_item(FocalGroupItem &g, const LMTask *t) {
    if (!t)
        return;
    pl_camera_pose *pose = static_cast<pl_camera_pose *>(g.item->model);
    double rec[kModelStride];
    if (t->skipped)
        record_from_pose(pose, false, rec);
    else
        record_from_lm_params(EST_ABS, t->params, rec); // (same inline function as the device)
    front_finish(g.fe, rec, &t->cam, pose, g.item->camera1);
}
// robust.cc:401-417: refine_shared_focal_relpose over the inliers, the focal length back in pixels
void focal_group_bundle_task(SFocalLMTask &t, FocalGroupItem &g) {
    std::memset(&t, 0, sizeof(t));
    for (int i = 0; i < 4; ++i)
        t.a[i] = g.prob.ps.a[i];
    t.n = g.n;
    for (int i = 0; i < 4; ++i)
        t.params[i] = g.best.q[i];
    for (int i = 0; i < 3; ++i)
        t.params[4 + i] = g.best.t[i];
    t.params[kSFocalFocalSlot] = g.best.f;
    t.opt = to_lm(g.fe.scaled.bundle);
    t.prefilter_thr2 = 0.0;
    t.mask = g.d_mask;
    t.scratch = nullptr;
}
void focal_group_finish_item(FocalGroupItem &g, const SFocalLMTask *t) {
    double f = g.best.f;
    if (t && !t->skipped) {
        pl_camera_pose *pose = static_cast<pl_camera_pose *>(g.item->model);
        for (int i = 0; i < 4; ++i)
            pose->q[i] = t->params[i];
        for (int i = 0; i < 3; ++i)
            pose->t[i] = t->params[4 + i];
        f = t->params[kSFocalFocalSlot];
    }
    g.item->camera1->params[0] = f * g.fe.scale; // :417
}

template <class P> int run_focal_group(Context *c, FocalGroupItem *const *pit, uint32_t count) {
    using Loop = FocalLoop<typename P::Traits>;
    using GenArgs = typename P::GenArgs;
    using ScoreArgs = typename P::ScoreArgs;
    using Task = typename P::Task;
    constexpr uint32_t kMaxModels = (uint32_t)P::Traits::kMaxModels, kSample = (uint32_t)P::Traits::kSample;
    if (count == 0)
        return PL_OK;
    if (!g_focal_group_ctx)
        g_focal_group_ctx = new FocalGroupContext();
    FocalGroupContext &gc = *g_focal_group_ctx;
    if (gc.device != c->device) { // (first use, or the thread's context was re-bound by pl_set_device)
        if (gc.device >= 0) {
            (void)hipSetDevice(gc.device);
            gc.release();
            HIP_TRY(hipSetDevice(c->device));
        }
        gc.device = c->device;
    }

    // ---- stage A ----
    const bool from_device = pit[0]->src_a != nullptr; // (a group is all-device or all-host)
    uint32_t max_n = 0;
    size_t raw_doubles = 0, pts_bytes = 0;
    std::vector<size_t> pts_off(count), raw_pts_off(count), mask_off(count);
    for (uint32_t i = 0; i < count; ++i) {
        FocalGroupItem &g = *pit[i];
        g.t_start = now_s();
        from_device ? focal_group_begin_device_item(g) : focal_group_prepare_item(g);
        max_n = std::max(max_n, g.n);
        g.raw_a_off = raw_doubles;
        raw_doubles += 2 * (size_t)g.n;
        g.raw_b_off = raw_doubles;
        raw_doubles += (size_t)P::kDb * g.n;
        pts_off[i] = pts_bytes;
        pts_bytes += align_up(sizeof(double) * P::kNd * g.n);
        if (P::kEst == 0) {
            raw_pts_off[i] = pts_bytes;
            pts_bytes += align_up(sizeof(double) * P::kNd * g.n);
        }
        mask_off[i] = pts_bytes;
        pts_bytes += align_up(g.n);
    }
    const uint32_t prep_entries = P::kEst == 0 ? 2 * count : count;
    // one table block, pinned and on the device: [prepare entries] at stage A, then per round [GenArgs | ScoreArgs (batches) | ScoreArgs
    // (refined models)], then [FocalMaskArgs] in the tail - every section at its own offset, uploaded with one copy
    const size_t sec_gen = 0, sec_score = align_up(sizeof(GenArgs) * count), sec_rscore = sec_score + align_up(sizeof(ScoreArgs) * count),
                 sec_end = sec_rscore + align_up(sizeof(ScoreArgs) * count);
    const size_t args_bytes = std::max({sizeof(PrepareGroupArgs) * prep_entries, sec_end, sizeof(FocalMaskArgs) * count});
    HIP_TRY(gc.pts.ensure(pts_bytes));
    HIP_TRY(gc.raw.ensure(sizeof(double) * raw_doubles));
    if (!from_device)
        HIP_TRY(gc.h_raw.ensure(sizeof(double) * raw_doubles));
    HIP_TRY(gc.args.ensure(args_bytes));
    HIP_TRY(gc.h_args.ensure(args_bytes));
    HIP_TRY(gc.h_mask.ensure(align_up(max_n) * count));
    if (from_device) {
        const int rc = focal_group_stage_device(c, gc, pit, count);
        if (rc != PL_OK)
            return rc;
    }
    {
        double *h_raw = gc.h_raw.as<double>();
        PrepareGroupArgs *hp = gc.h_args.as<PrepareGroupArgs>();
        CameraParams raw_cam;
        std::memset(&raw_cam, 0, sizeof(raw_cam));
        raw_cam.model_id = CAM_NULL; // pixels as they are
        for (uint32_t i = 0; i < count; ++i) {
            FocalGroupItem &g = *pit[i];
            if (!from_device) {
                std::memcpy(h_raw + g.raw_a_off, g.item->a, sizeof(double) * 2 * g.n);
                std::memcpy(h_raw + g.raw_b_off, g.item->b, sizeof(double) * P::kDb * g.n);
                g.raw_a = gc.raw.as<double>() + g.raw_a_off, g.raw_b = gc.raw.as<double>() + g.raw_b_off;
            }
            auto problem_at = [&](pl_problem &p, size_t off) {
                p.kind = P::kKind;
                p.device = c->device;
                p.n = g.n;
                p.d_pts = reinterpret_cast<double *>(gc.pts.as<char>() + off);
                p.borrowed = true;
                std::memset(&p.ps, 0, sizeof(p.ps));
                p.ps.n = g.n;
                for (int d = 0; d < P::kNd; ++d)
                    p.ps.a[d] = p.d_pts + (size_t)d * g.n;
                p.ps.xy_absmax = std::numeric_limits<float>::infinity();
            };
            auto entry = [&](PrepareGroupArgs &e, const PrepareArgs &pa, const pl_problem &p) {
                e.a_raw = g.raw_a;
                e.b_raw = g.raw_b;
                e.n = g.n;
                e.pad = 0;
                e.args = pa;
                e.soa = p.d_pts;
                e.absmax_bits = nullptr;
                e.stats = g.d_rec; // (device members: the scale comes from the record the launch in front of this one writes)
            };
            problem_at(g.prob, pts_off[i]);
            entry(hp[i], g.fe.prep, g.prob);
            if (P::kEst == 0) {
                problem_at(g.prob_raw, raw_pts_off[i]);
                entry(hp[count + i], prepare_unproject(raw_cam, nullptr), g.prob_raw);
            }
            g.d_mask = gc.pts.as<uint8_t>() + mask_off[i];
        }
        if (!from_device)
            HIP_TRY(hipMemcpyAsync(gc.raw.p, h_raw, sizeof(double) * raw_doubles, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(gc.args.p, hp, sizeof(PrepareGroupArgs) * prep_entries, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(launch_group_prepare(gc.args.as<PrepareGroupArgs>(), prep_entries, max_n, c->stream));
        // (the pinned table is rewritten below before the device has read it: wait - the first round's host work is short)
        HIP_TRY(wait_stream(c));
        if (from_device) // the stage's one synchronisation is behind us: the scales, and what the host forms from them
            for (uint32_t i = 0; i < count; ++i)
                focal_group_scale_from_device(*pit[i]);
    }

    // ---- the loops ----
    std::vector<std::unique_ptr<Loop>> loops(count);
    std::vector<char> active(count, 0);
    for (uint32_t i = 0; i < count; ++i) {
        FocalGroupItem &g = *pit[i];
        std::memset(g.st, 0, sizeof(*g.st));
        loops[i].reset(new Loop(g.n, g.lo, &g.best, &g.fs));
        active[i] = 1;
    }
    const size_t npad_max = ((size_t)max_n + 255u) & ~(size_t)255u;
    std::vector<uint32_t> min_members, ref_members;
    std::vector<char> waiting(count, 0); // a batch request that did not fit into its round's budget: served in a later round
    // The host's mirror of a batch is (4 + 4 + 8 + 64) bytes per model slot: 0.76 / 4.6 KB per iteration, and next to it the batch
    // holds its models, the generator's stage (8.8 KB per iteration for pnpf) and its positions on the device.  A round's batches
    // share one block of each; members whose batch would push their SUM past the budget wait for the next round (long batches of
    // hard problems: 4096 iterations x 64 members would be 600 MB of mirror and 2.3 GB of stage per worker - ADVICE r5: round 5
    // bounded the mirror only).  POSELIB_AMD_FOCAL_MIRROR_MB: a quarter of the budget (tests; default 192 -> 768 MB per worker).
    static const size_t round_budget = [] {
        const char *e = std::getenv("POSELIB_AMD_FOCAL_MIRROR_MB");
        return (size_t)4 * ((size_t)(e ? std::max<long>(std::atol(e), 1) : 192L) << 20);
    }();
    const size_t mirror_per_slot = 2 * sizeof(uint32_t) + sizeof(double) + sizeof(FocalModel);
    auto member_bytes = [&](uint32_t nb) { // pinned mirror + device workspace of ONE member's batch of nb iterations
        const size_t slots = (size_t)nb * kMaxModels;
        return slots * (mirror_per_slot + sizeof(FocalModel)) + (size_t)nb * sizeof(uint32_t) * (3 + kSample) + P::stage_bytes(nb);
    };
    for (;;) {
        // every running member to its next request
        min_members.clear();
        ref_members.clear();
        uint32_t max_B = 0, total_tasks = 0, max_tasks = 0;
        for (uint32_t i = 0; i < count; ++i) {
            if (!active[i])
                continue;
            FocalGroupItem &g = *pit[i];
            Loop &L = *loops[i];
            if (!waiting[i])
                g.request = (int)L.advance();
            switch (g.request) {
            case Loop::kDone:
                active[i] = 0;
                break;
            case Loop::kMinimal: {
                const uint32_t nb = std::max(max_B, L.B);
                waiting[i] = !min_members.empty() && (min_members.size() + 1) * member_bytes(nb) > round_budget;
                if (waiting[i])
                    break;
                min_members.push_back(i);
                max_B = nb;
                break;
            }
            case Loop::kRefineScore:
                g.task0 = total_tasks;
                g.ntasks = (uint32_t)L.seeds.size();
                total_tasks += g.ntasks;
                max_tasks = std::max(max_tasks, g.ntasks);
                ref_members.push_back(i);
                break;
            default: // kScore: only with score_initial_model, which this path does not take
                return fail(PL_ERR_INVALID, "focal group: unexpected request of the loop");
            }
        }
        if (min_members.empty() && ref_members.empty())
            break;
        char *h_args = gc.h_args.as<char>();
        char *d_args = gc.args.as<char>();
        // -- batches of iterations: per member [positions] in pinned memory, models / counts / workspace on the device, the host's
        //    mirror [counts u32 x slots | num_models u32 x B | sums f64 x slots | models x slots] written by the kernels themselves
        const uint32_t Gm = (uint32_t)min_members.size();
        const size_t slots_max = (size_t)max_B * kMaxModels;
        const size_t o_cnt = 0, o_nm = align_up(sizeof(uint32_t) * slots_max, 8), o_sum = o_nm + align_up(sizeof(uint32_t) * max_B, 8),
                     o_mod = o_sum + sizeof(double) * slots_max, out_stride = align_up(o_mod + sizeof(FocalModel) * slots_max);
        const size_t pos_stride = align_up(sizeof(uint32_t) * max_B), mod_stride = align_up(sizeof(FocalModel) * slots_max),
                     nm_stride = align_up(sizeof(uint32_t) * max_B), stage_stride = align_up(P::stage_bytes(max_B));
        const size_t smp_stride = align_up(sizeof(uint32_t) * (size_t)max_B * kSample);
        if (Gm) {
            HIP_TRY(gc.h_pos.ensure(pos_stride * Gm));
            bool any_prosac = false;
            for (uint32_t k = 0; k < Gm; ++k)
                any_prosac = any_prosac || loops[min_members[k]]->explicit_samples;
            if (any_prosac)
                HIP_TRY(gc.h_smp.ensure(smp_stride * Gm));
            HIP_TRY(gc.h_out.ensure(out_stride * Gm));
            HIP_TRY(gc.models.ensure(mod_stride * Gm));
            HIP_TRY(gc.num_models.ensure(nm_stride * Gm));
            HIP_TRY(gc.stage.ensure(stage_stride * Gm));
            GenArgs *hg = reinterpret_cast<GenArgs *>(h_args + sec_gen);
            ScoreArgs *hs = reinterpret_cast<ScoreArgs *>(h_args + sec_score);
            for (uint32_t k = 0; k < Gm; ++k) {
                FocalGroupItem &g = *pit[min_members[k]];
                Loop &L = *loops[min_members[k]];
                std::memcpy(gc.h_pos.as<char>() + pos_stride * k, L.positions.data(), sizeof(uint32_t) * L.B);
                char *d_out = gc.h_out.dev<char>() + out_stride * k;
                GenArgs &ga = hg[k];
                P::gen_args(ga, g);
                ga.n = g.n;
                ga.seed = g.lo.seed;
                ga.pos_base = L.pos;
                ga.positions = reinterpret_cast<const uint32_t *>(gc.h_pos.dev<char>() + pos_stride * k);
                ga.samples = nullptr;
                if (L.explicit_samples) { // PROSAC: the samples FocalLoop::advance drew for this batch
                    std::memcpy(gc.h_smp.as<char>() + smp_stride * k, L.prosac_samples.data(), sizeof(uint32_t) * (size_t)L.B * kSample);
                    ga.samples = reinterpret_cast<const uint32_t *>(gc.h_smp.dev<char>() + smp_stride * k);
                }
                ga.num_iters = L.B;
                ga.models = reinterpret_cast<FocalModel *>(gc.models.as<char>() + mod_stride * k);
                ga.num_models = reinterpret_cast<uint32_t *>(gc.num_models.as<char>() + nm_stride * k);
                ga.stage = reinterpret_cast<double *>(gc.stage.as<char>() + stage_stride * k);
                ga.explicit_in = nullptr;
                ga.host_models = reinterpret_cast<FocalModel *>(d_out + o_mod);
                ga.host_num_models = reinterpret_cast<uint32_t *>(d_out + o_nm);
                ScoreArgs &sa = hs[k];
                P::score_args(sa, g, nullptr, reinterpret_cast<uint32_t *>(d_out + o_cnt), reinterpret_cast<double *>(d_out + o_sum));
                sa.models = ga.models;
                sa.num_models = ga.num_models;
                sa.num_slots = L.B * kMaxModels;
            }
        }
        // -- local optimisations: the tasks of all members in one pinned block, their scores behind them
        const uint32_t Gr = (uint32_t)ref_members.size();
        if (Gr) {
            HIP_TRY(gc.h_tasks.ensure(sizeof(Task) * total_tasks));
            HIP_TRY(gc.h_rout.ensure((sizeof(uint32_t) + sizeof(double)) * total_tasks + 64));
            if (P::lo_needs_scratch())
                HIP_TRY(gc.lm_scratch.ensure(npad_max * total_tasks));
            Task *ht = gc.h_tasks.as<Task>();
            double *d_rsums = gc.h_rout.dev<double>();
            uint32_t *d_rcounts = reinterpret_cast<uint32_t *>(d_rsums + total_tasks);
            ScoreArgs *hs = reinterpret_cast<ScoreArgs *>(h_args + sec_rscore);
            for (uint32_t k = 0; k < Gr; ++k) {
                FocalGroupItem &g = *pit[ref_members[k]];
                Loop &L = *loops[ref_members[k]];
                for (uint32_t j = 0; j < g.ntasks; ++j)
                    P::lo_task(ht[g.task0 + j], g, L.seeds[j],
                               P::lo_needs_scratch() ? gc.lm_scratch.as<uint8_t>() + npad_max * (g.task0 + j) : nullptr);
                ScoreArgs &sa = hs[k];
                P::score_args(sa, g, gc.h_tasks.dev<Task>() + g.task0, d_rcounts + g.task0, d_rsums + g.task0);
                sa.models = nullptr;
                sa.num_models = nullptr;
                sa.num_slots = g.ntasks;
            }
        }
        HIP_TRY(hipMemcpyAsync(d_args, h_args, sec_end, hipMemcpyHostToDevice, c->stream));
        if (Gm) {
            HIP_TRY(P::generate(reinterpret_cast<const GenArgs *>(d_args + sec_gen), Gm, max_B, c->stream));
            HIP_TRY(P::score(reinterpret_cast<const ScoreArgs *>(d_args + sec_score), Gm, max_B * kMaxModels, false, c->stream));
        }
        if (Gr) {
            HIP_TRY(P::lm(gc.h_tasks.dev<Task>(), total_tasks, c->stream));
            HIP_TRY(P::score(reinterpret_cast<const ScoreArgs *>(d_args + sec_rscore), Gr, max_tasks, true, c->stream));
        }
        HIP_TRY(wait_stream(c));
        // -- the responses
        for (uint32_t k = 0; k < Gm; ++k) {
            Loop &L = *loops[min_members[k]];
            const char *h_out = gc.h_out.as<char>() + out_stride * k;
            const uint32_t *h_cnt = reinterpret_cast<const uint32_t *>(h_out + o_cnt), *h_nm = reinterpret_cast<const uint32_t *>(h_out + o_nm);
            const double *h_sum = reinterpret_cast<const double *>(h_out + o_sum);
            const FocalModel *h_mod = reinterpret_cast<const FocalModel *>(h_out + o_mod);
            const uint32_t B = L.B;
            L.num_models.assign(h_nm, h_nm + B);
            L.models.clear(), L.counts.clear(), L.sums.clear(); // (compact: one entry per model, in (iteration, slot) order)
            for (uint32_t b = 0; b < B; ++b)
                for (uint32_t m = 0; m < L.num_models[b]; ++m) {
                    const size_t h = (size_t)b * kMaxModels + m;
                    L.models.push_back(h_mod[h]);
                    L.counts.push_back(h_cnt[h]);
                    L.sums.push_back(h_sum[h]);
                }
        }
        if (Gr) {
            const Task *ht = gc.h_tasks.as<Task>();
            const double *h_rsums = gc.h_rout.as<double>();
            const uint32_t *h_rcounts = reinterpret_cast<const uint32_t *>(h_rsums + total_tasks);
            for (uint32_t k = 0; k < Gr; ++k) {
                FocalGroupItem &g = *pit[ref_members[k]];
                Loop &L = *loops[ref_members[k]];
                L.refined.resize(g.ntasks);
                for (uint32_t j = 0; j < g.ntasks; ++j)
                    P::lo_result(ht[g.task0 + j], L.seeds[j], L.refined[j]);
                L.rcounts.assign(h_rcounts + g.task0, h_rcounts + g.task0 + g.ntasks);
                L.rsums.assign(h_rsums + g.task0, h_rsums + g.task0 + g.ntasks);
            }
        }
    }
    (void)kSample;

    // ---- tail: get_inliers (ransac.cc:72 / 194-200), then the front-ends' bundles over the inliers ----
    {
        FocalMaskArgs *hm = gc.h_args.as<FocalMaskArgs>();
        const size_t mask_stride = align_up(max_n);
        for (uint32_t i = 0; i < count; ++i) {
            FocalGroupItem &g = *pit[i];
            stats_from_focal_loop(g.fs, g.st);
            focal_group_loop_result(g);
            FocalMaskArgs &ma = hm[i];
            std::memset(&ma, 0, sizeof(ma));
            for (int d = 0; d < P::kNd; ++d)
                ma.a[d] = g.prob.ps.a[d];
            ma.n = g.n;
            ma.model = g.best;
            ma.thr2 = g.thr2;
            ma.mask = g.d_mask;
            if (g.mdest) // the caller's device memory, written by the mask launch itself: no pinned mirror, nothing to copy out below
                ma.dst = g.mdest->data, ma.dst_stride = g.mdest->stride, ma.dst_order = g.mdest->order;
            else
                ma.host_mask = gc.h_mask.dev<uint8_t>() + mask_stride * i;
        }
        HIP_TRY(hipMemcpyAsync(gc.args.p, hm, sizeof(FocalMaskArgs) * count, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(P::mask(gc.args.as<FocalMaskArgs>(), count, max_n, c->stream));
        // the bundles (robust.cc:103-123 with the focal length free / :401-415 refine_shared_focal_relpose): tasks in the pinned block
        std::vector<int> task_of(count, -1);
        uint32_t nb = 0;
        for (uint32_t i = 0; i < count; ++i)
            if (pit[i]->st->num_inliers > front_min_inliers(P::kEst == 0 ? EST_ABS : kFrontSharedFocal))
                task_of[i] = (int)nb++;
        if (nb) {
            HIP_TRY(gc.h_tasks.ensure(sizeof(Task) * nb));
            Task *ht = gc.h_tasks.as<Task>();
            for (uint32_t i = 0; i < count; ++i) {
                if (task_of[i] < 0)
                    continue;
                FocalGroupItem &g = *pit[i];
                focal_group_bundle_task(ht[task_of[i]], g);
            }
            HIP_TRY(P::lm(gc.h_tasks.dev<Task>(), nb, c->stream));
        }
        HIP_TRY(wait_stream(c));
        const Task *ht = gc.h_tasks.as<Task>();
        for (uint32_t i = 0; i < count; ++i) {
            FocalGroupItem &g = *pit[i];
            if (g.item->inliers && g.n && !g.mdest)
                std::memcpy(g.item->inliers, gc.h_mask.as<uint8_t>() + mask_stride * i, g.n);
            focal_group_finish_item(g, task_of[i] >= 0 ? &ht[task_of[i]] : nullptr);
            g.st->seconds = now_s() - g.t_start;
            g.item->status = PL_OK;
        }
    }
    // (ADVICE r5) the first member of a round is admitted whatever its batch needs, and the buffers of a worker live as long as
    // its thread: a group that needed far more than a round's budget gives the memory back instead of pinning it for good
    if (gc.stage.cap + gc.models.cap + gc.num_models.cap + gc.h_out.cap > round_budget + ((size_t)64 << 20)) {
        for (DevBuf *b : {&gc.stage, &gc.models, &gc.num_models}) {
            if (b->p)
                (void)hipFree(b->p);
            b->p = nullptr, b->cap = 0;
        }
        if (gc.h_out.p)
            (void)hipHostFree(gc.h_out.p);
        gc.h_out.p = gc.h_out.dp = nullptr, gc.h_out.cap = 0;
    }
    return PL_OK;
}
