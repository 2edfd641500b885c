// poselib_amd — groups of problems through ONE launch sequence (included by driver.cc, inside its anonymous namespace).
//
// BASELINE config 4: thousands of independent image pairs with default options.  A default-options problem is ~10^3
// iterations - a few microseconds of device work per kernel - so worked through one problem at a time (one stream per
// problem, ~50 HIP API calls each) the HOST side of the runtime is the limit (round 1: 3300 problems/s however many
// streams).  Here up to kGroupMax problems of the same kind advance in lock-step: the problem index is a grid
// dimension of every kernel (blockIdx.z) and the per-problem arguments come from a device-resident table
// (GroupArgs), so a group costs the launches of ONE problem:
//
//   stage A  raw correspondences of all problems -> one pinned block -> one upload; k_prepare_g (un-projection /
//            normalisation, robust.cc:40-46, 286-292, utils.cc:584-644 per-point part).  Points in the caller's device memory
//            (pl_estimate_batch_dev): no pinned block and no upload - k_ingest_g, k_point_stats_g, then k_prepare_g
//   stage C  per batch step: positions, generate, compact, gather, score, finalize, records, candidates re-scored -
//            8..10 launches for the whole group, ONE synchronisation; the host replays every problem's sequential loop
//            (RansacRun: the same code as the single-problem path); all triggered local optimisations of all problems
//            as one k_lm launch + one re-scoring launch, ONE synchronisation
//   stage D  final refinement of the best model, choice refined / incumbent, inlier mask (ransac_impl.h:190-198) - one
//            launch each for the group
//   stage E  the front-ends' final non-linear refinement on the inliers (robust.cc:103-123, 296-311, 573-588, 736-751)
//
// The same machinery serves device-resident problems (pl_ransac_batch: `resident` groups skip stages A and E - the
// ransac_* contract - and may use batches of up to the full min_iterations when the arena budget allows: long fixed-length
// runs then are a handful of FAT launches per group instead of ~15 small ones per problem on 16 competing streams).
//
// Results are those of the single-problem entry points, bit for bit (same kernel bodies, same host replay):
// tests/test_gpu_group.py.  Problems the group path does not cover (PROSAC, warm starts, OPENCV cameras, fewer points
// than the sample, slot or candidate-list overflow, ...) are flagged and run through the single-problem path afterwards.

constexpr uint32_t kGroupMax = 128;         // problems per launch sequence: pl_ransac_batch's cap, pl_estimate_batch's default
constexpr uint32_t kGroupMaxAuto = 256;     // ... which grows with the size of the call up to this (driver.cc pl_estimate_batch)
constexpr uint32_t kGroupMaxPoints = 16384; // larger problems gain nothing from grouping

struct GroupLayout { // one slot of the arena (the same for every slot of a step): a batch step's buffers, then the group's own
    BatchSizes batch;
    size_t pts, pts2, mask, tmp_model, absmax, total; // byte offsets inside the slot
};

struct GroupContext { // per host thread AND device, kept for later groups
    int device = -1;  // the device every buffer below lives on (= Context::device of the thread when they were allocated)
    size_t budget = 0; // arena budget of this thread (bytes): its share when it sized its first group, lowered when the pools have grown since
    int budget_threads = 0; // number of pool threads on the device the budget was computed for
    DevBuf arena, raw, args, lm_records, lm_scratch, seq_count, seq_score, sel_count;
    HostBuf h_raw, h_args, h_ctl, h_meta, h_recm, h_offsets, h_mask, h_tasks, h_count, h_score, h_tail;
    HostBuf h_samples, h_absmax; // PROSAC samples of a step's members; max|x| read back from k_prepare_g (absolute pose through a non-linear camera)
    HostBuf h_raw_alt, h_prep_args;          // the NEXT group's raw points (staged while this worker waits for the device); stage A's table
    HostBuf h_ingest, h_pstats_args, h_pstats; // groups of pl_estimate_batch_dev: the tables of k_ingest_g / k_point_stats_g, the members' records
    const void *staged_first = nullptr;     // first item of the group whose raw points sit in h_raw_alt
    void release() { // pl_set_device moved the thread to another GPU: nothing of the old device may be reused
        for (DevBuf *b : {&arena, &raw, &args, &lm_records, &lm_scratch, &seq_count, &seq_score, &sel_count}) {
            if (b->p)
                (void)hipFree(b->p);
            b->p = nullptr, b->cap = 0;
        }
        staged_first = nullptr;
        for (HostBuf *b : {&h_raw, &h_args, &h_ctl, &h_meta, &h_recm, &h_offsets, &h_mask, &h_tasks, &h_count, &h_score, &h_tail, &h_raw_alt, &h_prep_args, &h_samples, &h_absmax, &h_ingest, &h_pstats_args, &h_pstats}) {
            if (b->p)
                (void)hipHostFree(b->p);
            b->p = b->dp = nullptr, b->cap = 0;
        }
        budget = 0;
    }
};
thread_local GroupContext *g_group_ctx = nullptr;
// High-water marks over ALL workers of the process (bytes): which worker serves which group differs from call to call, and a worker whose
// buffers are smaller than the group it gets re-allocates (hipFree + hipMalloc / hipHostMalloc: a device-wide stall of 10 - 100 ms).  Every
// worker therefore sizes its non-resident group buffers to the largest any worker has needed so far: steady state from the second call on.
std::atomic<size_t> g_hw_arena{0}, g_hw_raw{0}, g_hw_tasks{0}, g_hw_lm_scratch{0}, g_hw_mask{0};
inline size_t raise_hw(std::atomic<size_t> &hw, size_t v) {
    size_t cur = hw.load(std::memory_order_relaxed);
    while (cur < v && !hw.compare_exchange_weak(cur, v, std::memory_order_relaxed)) {
    }
    return std::max(cur, v);
}
// Batch sizes of a group's members (pl_estimate_batch).  A single problem's run doubles its batches (1024, 2048, 4096, ...: the waste
// of a speculative batch stays below 2 x); in a group a STEP costs ~1 ms of dependent launches whatever its members' batch sizes, and
// a call of a few hundred problems is as long as its longest member's chain of steps.  So from the second step on a member asks for
// what its loop is known to need (the stop rule's bound after the first local optimisations, RansacRun::needed_now) up to this
// capacity: the 5-point problems with 60 - 70 % outliers (~4 - 10 k iterations) finish in two steps instead of five.  Measured
// (profiles/r06_batch_sizes.md): 512 problems per call 48.8 -> 59.8 k problems/s, 4096 per call unchanged (82 k).  The outcome does
// not depend on how the iterations are cut into batches (the replay is exact).
constexpr uint32_t kGroupJump = 8192;
// worker threads of the batch pools, per device: they are persistent and keep their arenas for the life of the process, so the
// arena budget of a thread is its share of what ALL of them may hold (several pl_*_batch calls can be in flight - four pools per
// device - and their workers' budgets must not add up to more than the device has: ADVICE r5)
constexpr int kMaxDevices = 64;
std::atomic<int> g_pool_threads[kMaxDevices];
// POSELIB_AMD_GROUP_TIMING: host phases of run_group (ns, summed over the workers of a call)
std::atomic<uint64_t> g_t_stageA{0}, g_t_args{0}, g_t_imp{0}, g_t_lmtasks{0}, g_t_replay{0}, g_t_tail{0};
double g_t_call0 = 0; // (diagnostic) start of the batch call the chain lines of POSELIB_AMD_GROUP_TIMING are relative to
struct PhaseTimer {
    std::atomic<uint64_t> &acc;
    double t0;
    explicit PhaseTimer(std::atomic<uint64_t> &a) : acc(a), t0(g_group_timing ? now_s() : 0.0) {}
    ~PhaseTimer() {
        if (g_group_timing)
            acc += (uint64_t)((now_s() - t0) * 1e9);
    }
}; // host threads of the running pl_*_batch call (sizes their arena budgets)
// the first error message of a worker of a batch call (the workers' g_err is thread-local).  One slot per worker pool - a call
// leases a pool for its duration, so calls in flight at the same time do not read or wipe each other's message (ADVICE r5); a
// worker finds its pool's slot through g_err_slot, set when the pool starts the thread.
struct WorkerError {
    std::mutex mu;
    std::string msg;
    std::atomic<uint64_t> fallbacks{0}; // items a group handed back to the single-problem path during the current call
    void note(const std::string &e) {
        std::lock_guard<std::mutex> lk(mu);
        if (msg.empty())
            msg = e;
    }
    std::string take() {
        std::lock_guard<std::mutex> lk(mu);
        std::string e;
        e.swap(msg);
        return e;
    }
};
thread_local WorkerError *g_err_slot = nullptr;
void note_worker_error() {
    if (g_err_slot)
        g_err_slot->note(g_err);
}
void note_fallback_item() {
    if (g_err_slot)
        g_err_slot->fallbacks.fetch_add(1);
}
// what the calling thread's last batch call did with its items (pl_last_batch_report)
thread_local pl_batch_report g_last_report = {0, 0, 0, 0, 0};

struct GroupItem {
    pl_batch_item *item = nullptr;
    const pl_batch_item_dev *ditem = nullptr; // pl_estimate_batch_dev: the caller's item, whose points are in device memory (`item`: its
                                              // host-side copy with a == b == null; nothing of a group reads host points then)
    pl_ransac_item *ritem = nullptr; // device-resident problem (pl_ransac_batch) instead of `item`
    int kind = 0;
    uint32_t n = 0;
    FrontEnd fe;                // the front-end's options, normalisation and final bundle (resident problems: the options alone)
    CameraParams cam_refined;   // abs, fe.cam_flags != 0: the rescaled camera after the bundle
    pl_problem prob;            // borrowed SoA block in the arena
    double rec[kModelStride];   // best model record
    pl_ransac_stats local_st;
    pl_ransac_stats *st = nullptr;
    RansacRun *run = nullptr;
    RansacRun::Batch b;
    bool active = false;   // takes part in the current batch step
    bool fallback = false; // run through the single-problem path afterwards
    bool looped = false;   // N >= sample size: the loop ran
    uint32_t job0 = 0;
    uint32_t job_e = 0; // index of the item's final-bundle task when that is enqueued behind stage D (merged tail)
    bool prepared = false; // group_prepare_item has run (by the staging hook)
    bool have_absmax = false; // ... and the bound of max|x| of the un-projected points (a host pass over the points)
    float xy_absmax = 0.f;
    bool deferred = false; // still running after the group's step budget: continues in a regrouped call (run_group `resume`)
    int64_t off_fetch = -1; // entry of the slot's offsets table whose value (hypotheses up to the stop) stage D fetches
    size_t raw_a_off = 0, raw_b_off = 0; // offsets (doubles) into the group's raw block
    const double *raw_a = nullptr, *raw_b = nullptr; // the member's fp64 AoS blocks on the device: its slices of the raw block, or -
                                                     // contiguous fp64 sets of a pl_estimate_batch_dev item - the caller's memory
    double t_start = 0;
    const MaskDest *mdest = nullptr; // pl_estimate_batch_dev_masked: the item's inlier mask goes to the caller's device memory - stage
                                     // D's mask launch writes it there, the member has no slice of the pinned mask block
    uint32_t hmask_slot = 0;         // ... every other member's slice of that block
};

size_t align_up(size_t v, size_t a = 256) { return (v + a - 1) / a * a; }

// points_on_device: an item of pl_estimate_batch_dev (its descriptors have been checked; a and b are null)
bool group_eligible(const pl_batch_item &it, bool points_on_device = false) {
    if (it.kind < 0 || it.kind > 3 || !it.opt || !it.model || (!points_on_device && (!it.a || !it.b)))
        return false;
    const pl_robust_options &o = *it.opt;
    if (validate_options(&o) != PL_OK)
        return false;
    // (round 6: PROSAC - the member's samples are drawn on the host step by step -, warm starts - the initial model is scored and
    // refined on the worker's stream before the lock-step loop - and non-linear cameras (OPENCV, SIMPLE_RADIAL, RADIAL, the fisheye models) of absolute-pose problems - max|x| of the
    // un-projected points rides stage A's read-back - are group members like any other)
    if (it.n < (size_t)sample_size(it.kind) + 4 || it.n > kGroupMaxPoints)
        return false;
    if (o.ransac.max_iterations == 0 || o.ransac.min_iterations > 4096)
        return false; // long fixed-length runs are device-bound on their own: one stream per problem serves them
    if (it.kind == EST_ABS) {
        if (!it.camera1 || !camera_supported(it.camera1))
            return false;
    }
    if (it.kind == EST_REL) {
        if (!it.camera1 || !it.camera2 || !camera_supported(it.camera1) || !camera_supported(it.camera2))
            return false;
    }
    return true;
}

bool group_eligible_resident(const pl_ransac_item &it) {
    if (!it.problem || !it.opt || !it.model)
        return false;
    const pl_problem &p = *it.problem;
    const pl_robust_options &o = *it.opt;
    if (p.kind < 0 || p.kind > 3 || validate_options(&o) != PL_OK)
        return false;
    if (o.ransac.max_iterations == 0)
        return false;
    if (p.n < (uint32_t)sample_size(p.kind) + 4 || p.n > kGroupMaxPoints)
        return false;
    return true;
}

// A batch step's buffers packed one behind the other from `base`, 256-byte aligned each; returns the bytes they take (base ==
// nullptr: only that).  The pinned mirrors are the caller's.
size_t pack_batch_buffers(char *base, const BatchSizes &z, BatchBuffers &b) {
    size_t o = 0;
    auto take = [&](auto *&ptr, size_t bytes) {
        ptr = reinterpret_cast<std::remove_reference_t<decltype(ptr)>>(reinterpret_cast<uintptr_t>(base) + o);
        o += align_up(bytes);
    };
    take(b.positions, z.positions);
    take(b.delta, z.delta);
    take(b.flags, z.flags);
    take(b.samples, z.samples);
    take(b.models, z.models);
    take(b.num_models, z.num_models);
    take(b.nan_bits, z.nan_bits);
    take(b.slots, z.slots);
    take(b.offsets, z.offsets);
    take(b.ctl, z.ctl);
    take(b.shadow, z.shadow);
    take(b.compact64, z.compact64);
    take(b.shadow16, z.shadow16);
    take(b.live, z.live);
    take(b.rank, z.rank);
    take(b.points16, z.points16);
    take(b.part_count, z.part_count);
    take(b.part_score, z.part_score);
    take(b.count, z.count);
    take(b.score, z.score);
    take(b.blk_best, z.blk_best);
    take(b.rec_meta, z.rec_meta);
    take(b.rec_models, z.rec_models);
    take(b.gen_stage, z.gen_stage);
    take(b.prune_sel, z.prune_sel);
    take(b.prune_kept, z.prune_kept);
    take(b.prune_state, z.prune_state);
    return o;
}

// max_B iterations, a sampler window of max_M, maxm record slots per iteration, `chunks` chunks of 64 P correspondences (P: the
// group's points per lane): room for every member, whichever scorer it turns out to use (batch_step_sizes)
GroupLayout group_layout(int kind, uint32_t max_n, uint32_t max_B, uint32_t max_M, uint32_t maxm, uint32_t chunks,
                         bool resident = false) {
    GroupLayout L;
    BatchShape s;
    s.B = s.Bl = max_B, s.lo = 0, s.M = max_M, s.slots = maxm, s.chunks = chunks;
    s.point_rows = chunks * 64u * (uint32_t)group_points_per_lane(kind);
    s.use_mfma = true;
    L.batch = batch_step_sizes(kind, s);
    BatchBuffers unused;
    size_t o = pack_batch_buffers(nullptr, L.batch, unused);
    auto take = [&](size_t bytes) {
        const size_t at = o;
        o += align_up(bytes);
        return at;
    };
    const int nd = point_doubles(kind);
    L.pts = take(resident ? 0 : sizeof(double) * nd * max_n);
    L.pts2 = take(kind == EST_ABS && !resident ? sizeof(double) * nd * max_n : 0);
    L.mask = take(max_n);
    L.tmp_model = take(sizeof(double) * kModelStride);
    L.absmax = take(sizeof(unsigned long long));
    L.total = align_up(o, 4096);
    return L;
}

// ---- stage A: per-item front-end arithmetic on the host (robust.cc), raw points into the pinned block ----
int group_prepare_item(GroupItem &g) {
    pl_batch_item &it = *g.item;
    g.kind = it.kind;
    g.n = (uint32_t)it.n;
    g.st = it.stats ? it.stats : &g.local_st;
    front_begin(g.fe, it.kind, it.a, it.b, it.n, *it.opt, it.camera1, it.camera2);
    return PL_OK;
}

// ... of an item whose points are in device memory: what run_group sizes the group by; the front-end itself follows in stage A,
// from the record k_point_stats_g writes (group_stage_device, driver_dev.inc)
int group_prepare_device_item(GroupItem &g) {
    const pl_batch_item &it = *g.item;
    g.kind = it.kind;
    g.n = (uint32_t)it.n;
    g.st = it.stats ? it.stats : &g.local_st;
    g.fe.kind = it.kind;
    g.fe.scaled = *it.opt;
    return PL_OK;
}
bool reads_in_place(const pl_device_points *d);
int group_stage_device(Context *c, GroupContext &gc, GroupItem *const *pit, uint32_t count, bool resume);

int group_prepare_resident(GroupItem &g) {
    pl_ransac_item &it = *g.ritem;
    g.kind = it.problem->kind;
    g.n = it.problem->n;
    g.st = it.stats ? it.stats : &g.local_st;
    g.fe = FrontEnd();
    g.fe.kind = g.kind;
    g.fe.scaled = *it.opt;
    return PL_OK;
}

// the bound of max(|x|, |y|) of an item's prepared points (+inf while stage A has still to read it back from the device)
float group_item_absmax(const GroupItem &g) {
    if (prefilter_bound_on_device(g.kind, g.fe.prep))
        return std::numeric_limits<float>::infinity();
    return host_prefilter_bound(g.kind, g.fe.prep, g.item->a, g.item->b, g.n);
}

// The host half of stage A for a group this worker will run NEXT, done while it waits for the device with the current group: the
// per-item front-end arithmetic (group_prepare_item) and the copy of the raw correspondences into the alternate pinned block
// (0.1 MB per problem: 40 ms of memcpy per call of 4096 problems, 13 % of the workers' time when it sat in front of every group).
void group_stage_in(GroupItem *const *pit, uint32_t count) {
    if (count == 0 || !g_group_ctx)
        return;
    GroupContext &gc = *g_group_ctx;
    const int db = ((*pit[0]).kind == EST_ABS) ? 3 : 2;
    size_t raw_doubles = 0;
    for (uint32_t i = 0; i < count; ++i) {
        GroupItem &g = (*pit[i]);
        group_prepare_item(g);
        g.prepared = true;
        g.xy_absmax = group_item_absmax(g);
        g.have_absmax = true;
        g.raw_a_off = raw_doubles;
        raw_doubles += 2 * (size_t)g.n;
        g.raw_b_off = raw_doubles;
        raw_doubles += (size_t)db * g.n;
    }
    if (gc.h_raw_alt.ensure(raise_hw(g_hw_raw, sizeof(double) * std::max<size_t>(raw_doubles, 1))) != hipSuccess) {
        (void)hipGetLastError();
        return; // (stage A copies as before)
    }
    double *h = gc.h_raw_alt.as<double>();
    for (uint32_t i = 0; i < count; ++i) {
        GroupItem &g = (*pit[i]);
        std::memcpy(h + g.raw_a_off, g.item->a, sizeof(double) * 2 * g.n);
        std::memcpy(h + g.raw_b_off, g.item->b, sizeof(double) * db * g.n);
    }
    gc.staged_first = pit[0];
}

// Hypothesis slices per chunk of correspondences of one member of a grouped scorer launch (workgroups of the member = slices x
// chunks).  Pure host arithmetic.  `hexp`: hypotheses the member's batch of `B` iterations is expected to hold, `chunks`: its
// chunks of correspondences, `launch_chunks`: the chunks of ALL active members of the launch (the member's own included).
//
// A member alone in its launch (`solo`): every workgroup (8 wavefronts) pays the operand split of its chunk, so a wavefront should
// see about three units of 64 hypotheses - 24 units per workgroup.  The list is shorter than its capacity: P3P fills 1.3 of 4 slots
// per iteration (sized by capacity, a group of 228 default-option problems launched 21 888 workgroups of which two thirds of the
// wavefronts found no unit: 2.0 ms per step).  k_score_mfma (absolute pose on the matrix cores) reads the operand rows of its
// chunk from the problem's table instead of splitting them: 48 units per workgroup (profiles/live_hypotheses.md).
//
// k_score_mfma_g, many members: the launch as a whole should come to about kGroupScoreWorkgroups workgroups, however many
// members share it - slices = ceil(kGroupScoreWorkgroups / launch_chunks), never more than `solo`, never less than one per
// (member, chunk).  A full group of long runs (the flagship: 16 members x 16 chunks x 49 slices = 12 544 workgroups for 512
// resident slots, a workgroup's LDS held until its slowest wavefront is done) gets fewer, longer-lived workgroups; a launch with
// few members, or short lists, keeps exactly what it had.  No count depends on the slice count, and no decision: every (chunk,
// hypothesis) partial comes from one wavefront, whichever it is, and candidates are re-scored sequentially.  The last bits of a
// tree-order score can: a hypothesis's terms are added up per drain batch of its unit's queue, where a batch ends depends on the
// unit's other hypotheses, and the tail rule of unit_of_ticket cuts the end of the list into units of 16, 32 or 64 by the number
// of wavefronts per chunk (a hypothesis in the same unit under two slice counts gets the same bits; measured otherwise: one unit
// in the last place, tests/test_gpu_score_stream.py).  Where kGroupScoreWorkgroups comes from: profiles/group_slices.md.  The other scorers
// (two-view, homography, fp32 queue, tangent, 1D-radial) still split per workgroup and keep `solo`.
constexpr uint32_t kGroupScoreWorkgroups = 3328;
static uint32_t group_score_slices(int kind, bool use_mfma, size_t hexp, uint32_t B, uint32_t chunks, uint32_t launch_chunks) {
    const size_t units = (use_mfma && kind == EST_ABS) ? 48 : 24; // 64-hypothesis units per workgroup (8 wavefronts)
    uint32_t solo = std::max<uint32_t>(1u, std::min<uint32_t>((uint32_t)((hexp / 64 + units - 1) / units), 1536u / chunks));
    if (use_mfma && (kind == EST_REL || kind == EST_FUND)) // (every workgroup pays the fp16 split of its chunk: at least ~4 units of 64 hypotheses per wave)
        solo = std::max<uint32_t>(1u, std::min<uint32_t>({solo, 512u / chunks, B / 2048u + 1u}));
    if (!(use_mfma && kind == EST_ABS))
        return solo;
    launch_chunks = std::max(launch_chunks, chunks);
    return std::max<uint32_t>(1u, std::min<uint32_t>((kGroupScoreWorkgroups + launch_chunks - 1) / launch_chunks, solo));
}
// Which batch steps of a GROUP score in two phases (PruneArgs in pl_kernels.h; DESIGN.md section 4): the matrix-core absolute-pose
// scorer, when the step is long enough for four more small launches to be nothing and the lead to be a small part of its list - at
// least kPruneMinIterations iterations - and when there is a chunk to save: at least kPruneMinChunks chunks of correspondences.  Both
// are known on the host before the step; nothing else decides (no option, no environment variable).  Default-option problems (batches
// of 512 ... 4096 iterations) and problems of fewer than three chunks keep the single launch.  So does the single-problem path
// (RansacRun::enqueue_batch): a group's launch is several resident rounds of workgroups, so workgroups that return at once make room
// for others; the single launch is one round, and there the pruned form measured slower.
constexpr uint32_t kPruneMinIterations = 8192, kPruneMinChunks = 3;
bool score_prune_gate(int kind, bool use_mfma, uint32_t iterations, uint32_t chunks) {
    return kind == EST_ABS && use_mfma && iterations >= kPruneMinIterations && chunks >= kPruneMinChunks;
}
// The rule's inputs for one member, shared by run_group and pl_debug_group_slices:
// record slots per iteration.  5-point: up to 40 poses are possible, the single-problem path starts with 8 and repeats a batch
// with 40 when an iteration overflows (about one iteration in 2000 does: most default-option problems would leave the group);
// 16 here, overflow = fallback.  The slot count only moves records around: same results.
static uint32_t group_record_slots(int kind) { return (kind == EST_REL) ? 16u : (uint32_t)max_models(kind); }
// chunks of correspondences: 64 P per chunk, or 32 PG = 64 Pm on the matrix-core Sampson form
static uint32_t group_member_chunks(int kind, bool use_mfma, uint32_t n) {
    const int P = (use_mfma && (kind == EST_REL || kind == EST_FUND)) ? group_mfma2_points_per_lane(kind) : group_points_per_lane(kind);
    return std::max<uint32_t>(1u, (n + 64 * P - 1) / (64 * P));
}
// hypotheses a batch of B iterations is expected to hold (absolute pose: P3P fills 1.3 of its 4 slots; the others: capacity)
static size_t group_expected_hypotheses(int kind, uint32_t B, size_t hcap) {
    return (kind == EST_ABS) ? std::min<size_t>(hcap, (size_t)B + B / 2) : hcap;
}
// pl_debug_group_slices: the rule for one member of `n_points` correspondences and a batch of `iterations` iterations.  The one
// input it cannot know is whether the member's scorer is the matrix-core one: run_group asks score_uses_mfma with the problem's
// prefilter; here the prefilter of a problem with in-range coordinates and threshold is ASSUMED (ones in the fields
// score_uses_mfma reads), so the size, the kind and POSELIB_AMD_NO_MFMA decide.
static int debug_group_slices(int kind, uint32_t n_points, uint32_t iterations, uint32_t launch_chunks) {
    PrefilterArgs pf{};
    pf.enabled = 1;
    pf.g16 = pf.t16 = pf.h16 = 1.0f, pf.thr = 1.0f;
    const bool mfma = score_uses_mfma(kind, n_points, pf);
    const size_t hcap = (size_t)iterations * group_record_slots(kind);
    return (int)group_score_slices(kind, mfma, group_expected_hypotheses(kind, iterations, hcap), iterations,
                                   group_member_chunks(kind, mfma, n_points), launch_chunks);
}

// One group: `count` items of the same kind.  Items the path cannot finish get fallback = true.
// `max_steps` > 0: at most so many batch steps; problems that are still running then are DEFERRED (g.deferred: their RansacRun is
// kept, stages D / E skip them) - pl_estimate_batch regroups the deferred problems of all groups and calls again with `resume`
// (stage A uploads their points again, stage B keeps the runs), now with batches of up to 32768 iterations: the few long runs of a
// call - 5-point problems with 60 - 70 % outliers need ~10^4 iterations - no longer keep their whole group in lock-step for six
// more steps of 4096.
int run_group(Context *c, GroupItem *const *pit, uint32_t count, bool resident = false, uint32_t max_steps = 0, bool resume = false) {
    if (count == 0)
        return PL_OK;
    if (!g_group_ctx)
        g_group_ctx = new GroupContext();
    GroupContext &gc = *g_group_ctx;
    if (gc.device != c->device) { // (first use, or the thread's context was re-bound by pl_set_device)
        if (gc.device >= 0) {
            (void)hipSetDevice(gc.device);
            gc.release();
            HIP_TRY(hipSetDevice(c->device));
        }
        gc.device = c->device;
    }
    const int kind = (*pit[0]).kind;
    const int K = sample_size(kind);
    const int P = group_points_per_lane(kind);
    const int nd = point_doubles(kind), db = (kind == EST_ABS) ? 3 : 2;
    const double t_group = now_s();

    // ---- sizes ----
    uint32_t max_n = 0, max_B = 0;
    size_t raw_doubles = 0;
    for (uint32_t i = 0; i < count; ++i) {
        GroupItem &g = (*pit[i]);
        max_n = std::max(max_n, g.n);
        uint64_t grow = std::max<uint64_t>(g.fe.scaled.ransac.min_iterations + 2, 512);
        if (resume && g.run)
            grow = std::max<uint64_t>(grow, g.run->needed_now());
        grow = (grow + 63) / 64 * 64;
        // the batches of a run double in size; in a group they stop growing at the slot's capacity (the outcome does not
        // depend on how the iterations are cut into batches: the replay is exact)
        // (resident groups: long fixed-length runs are welcome - up to the whole run in one batch, arena permitting)
        max_B = std::max<uint32_t>(max_B, (uint32_t)std::min<uint64_t>(std::max<uint64_t>(grow, resident ? 2048 : kGroupJump), resident ? 131072 : (resume ? 32768 : kGroupJump)));
        if (!resident) { // (a device set that is contiguous fp64 is read where it lies: no slice)
            g.raw_a_off = raw_doubles;
            raw_doubles += (g.ditem && reads_in_place(&g.ditem->a)) ? 0 : 2 * (size_t)g.n;
            g.raw_b_off = raw_doubles;
            raw_doubles += (g.ditem && reads_in_place(&g.ditem->b)) ? 0 : (size_t)db * g.n;
        }
    }
    const bool from_device = !resident && (*pit[0]).ditem != nullptr; // (a group is all-device or all-host: pl_estimate_batch_dev)
    const uint32_t maxm = group_record_slots(kind); // record slots per iteration
    // the sampler window (sampler_window) is largest for the smallest problem of the group - the same function sizes every item's
    // window below (M64), so no item of a full-size batch outgrows the slot
    uint32_t min_n = (*pit[0]).n;
    for (uint32_t i = 1; i < count; ++i)
        min_n = std::min(min_n, (*pit[i]).n);
    // chunks of correspondences: 64 P per chunk, or 32 PG on the matrix-core Sampson form (the larger count sizes the arena)
    const int Pm = (kind == EST_REL || kind == EST_FUND) ? group_mfma2_points_per_lane(kind) : P;
    const uint32_t max_chunks = std::max<uint32_t>(1u, (max_n + 64 * std::min(P, Pm) - 1) / (64 * std::min(P, Pm)));
    // arena budget of this host thread: POSELIB_AMD_GROUP_ARENA_MB, else an equal share of 60 % of the memory that is FREE
    // on the device when the thread sizes its first resident group - a share among ALL worker threads of the device's batch
    // pools (g_pool_threads: several calls can be in flight) -, at most 12 GB, at least 256 MB: a second process on the
    // device, 64 workers, or four calls at once no longer add up to more than the device has
    static const long env_mb = [] {
        const char *e = std::getenv("POSELIB_AMD_GROUP_ARENA_MB");
        return e ? std::max<long>(std::atol(e), 256) : 0L;
    }();
    const int pool_threads = std::max(1, g_pool_threads[c->device & (kMaxDevices - 1)].load());
    if (gc.budget == 0 || (!env_mb && gc.budget_threads < pool_threads)) {
        gc.budget_threads = pool_threads;
        if (env_mb) {
            gc.budget = (size_t)env_mb << 20;
        } else {
            size_t free_b = 0, total_b = 0;
            if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) {
                (void)hipGetLastError();
                free_b = (size_t)16 << 30;
            }
            // (free memory + what this thread holds already; the other threads' arenas are not free any more, so a thread that
            // re-computes its share after the pools have grown can only come out lower)
            const size_t share = std::max<size_t>((size_t)256 << 20, (size_t)(0.6 * (double)(free_b + gc.arena.cap)) / (size_t)pool_threads);
            gc.budget = std::min<size_t>((size_t)12288 << 20, gc.budget ? std::min(gc.budget, share) : share);
        }
    }
    const size_t arena_budget = gc.budget;
    uint32_t max_M = 0;
    GroupLayout L;
    for (;;) {
        max_M = (uint32_t)sampler_window(min_n, K, max_B);
        L = group_layout(kind, max_n, max_B, max_M, maxm, max_chunks, resident);
        if (L.total * count <= arena_budget || max_B <= 4096)
            break;
        max_B = std::max<uint32_t>(4096u, (max_B / 2 + 63) / 64 * 64); // shorter batches, more of them: same results
    }
    {
        size_t want = L.total * count;
        if (!resident) { // (resident groups are sized by the budget; host-resident ones are small: share the high-water mark)
            const size_t hw = raise_hw(g_hw_arena, want);
            if (hw <= arena_budget)
                want = hw;
        }
        HIP_TRY(gc.arena.ensure(want));
    }
    bool staged = !resident && !from_device && gc.staged_first == (const void *)pit[0];
    if (staged) // the raw points were copied into the alternate block while this worker waited for its previous group
        std::swap(gc.h_raw, gc.h_raw_alt);
    gc.staged_first = nullptr;
    // test hook (tests/test_gpu_group.py): POSELIB_AMD_DEBUG_RAISE_RAW_HW = bytes by which "another worker" raises the
    // high-water mark between the staging of a group and its run - makes the re-allocation case below deterministic
    static const size_t debug_raise = [] {
        const char *e = std::getenv("POSELIB_AMD_DEBUG_RAISE_RAW_HW");
        return e ? (size_t)std::strtoull(e, nullptr, 10) : (size_t)0;
    }();
    if (debug_raise && staged)
        raise_hw(g_hw_raw, g_hw_raw.load(std::memory_order_relaxed) + debug_raise);
    const size_t raw_bytes = raise_hw(g_hw_raw, sizeof(double) * std::max<size_t>(raw_doubles, 1));
    // (ADVICE r4, high) the staged block was sized to the high-water mark AT STAGING TIME; another worker may have raised
    // the mark since, and HostBuf::ensure re-allocates WITHOUT keeping the contents - the staged points would be lost and
    // uninitialised pinned memory uploaded as this group's correspondences.  Such a block is not taken as staged: stage A
    // copies the caller's points again into the fresh allocation.
    if (staged && gc.h_raw.cap < raw_bytes)
        staged = false;
    HIP_TRY(gc.raw.ensure(raw_bytes));
    if (!from_device) // (no pinned staging block for points that are on the device already)
        HIP_TRY(gc.h_raw.ensure(raw_bytes));
    HIP_TRY(gc.h_prep_args.ensure(sizeof(PrepareGroupArgs) * count));
    const size_t args_bytes = std::max({sizeof(GroupArgs), sizeof(PrepareGroupArgs), sizeof(SeqScoreArgs) + sizeof(SelectArgs) + sizeof(MaskArgs)}) * count;
    HIP_TRY(gc.args.ensure(args_bytes));
    HIP_TRY(gc.h_args.ensure(args_bytes));
    HIP_TRY(gc.h_ctl.ensure(sizeof(BatchCtl) * count));
    HIP_TRY(gc.h_meta.ensure(sizeof(RecordMeta) * kRecordFirst * count));
    HIP_TRY(gc.h_recm.ensure(sizeof(double) * kModelStride * kRecordFirst * count));
    HIP_TRY(gc.h_offsets.ensure(sizeof(uint32_t) * (size_t)count));
    uint32_t host_masks = 0; // members whose mask comes back to the host
    for (uint32_t i = 0; i < count; ++i)
        if (!(*pit[i]).mdest)
            (*pit[i]).hmask_slot = host_masks++;
    HIP_TRY(gc.h_mask.ensure(resident ? (size_t)max_n * host_masks : raise_hw(g_hw_mask, (size_t)max_n * host_masks)));
    char *const arena = gc.arena.as<char>();
    auto slot = [&](uint32_t i, size_t off) { return arena + (size_t)i * L.total + off; };
    auto slot_buffers = [&](uint32_t i) { // member i's buffers of a batch step and the pinned mirrors of its small results
        BatchBuffers b;
        pack_batch_buffers(slot(i, 0), L.batch, b);
        b.host_meta = gc.h_meta.dev<RecordMeta>() + (size_t)i * kRecordFirst;
        b.host_models = gc.h_recm.dev<double>() + (size_t)i * kRecordFirst * kModelStride;
        b.host_ctl = gc.h_ctl.dev<BatchCtl>() + i;
        return b;
    };

    // ---- stage A: raw points -> pinned block -> device; k_prepare_g (resident problems: their own SoA block) ----
    std::unique_ptr<PhaseTimer> ptA(new PhaseTimer(g_t_stageA));
    if (resident) {
        for (uint32_t i = 0; i < count; ++i) {
            GroupItem &g = (*pit[i]);
            g.prob = *g.ritem->problem; // (pointers into the user's pl_problem; nothing here is freed through this copy)
            g.prob.borrowed = true;
        }
    } else {
        uint32_t n_dev_absmax = 0;
        if (from_device) { // k_ingest_g, k_point_stats_g, the members' front-ends: no host copy of points
            const int rc = group_stage_device(c, gc, pit, count, resume);
            if (rc != PL_OK)
                return rc;
        } else {
            double *h_raw = gc.h_raw.as<double>();
            if (!staged)
                for (uint32_t i = 0; i < count; ++i) {
                    GroupItem &g = (*pit[i]);
                    std::memcpy(h_raw + g.raw_a_off, g.item->a, sizeof(double) * 2 * g.n);
                    std::memcpy(h_raw + g.raw_b_off, g.item->b, sizeof(double) * db * g.n);
                }
            HIP_TRY(hipMemcpyAsync(gc.raw.p, h_raw, sizeof(double) * raw_doubles, hipMemcpyHostToDevice, c->stream));
            for (uint32_t i = 0; i < count; ++i) {
                GroupItem &g = (*pit[i]);
                g.raw_a = gc.raw.as<double>() + g.raw_a_off;
                g.raw_b = gc.raw.as<double>() + g.raw_b_off;
            }
        }
        PrepareGroupArgs *hp = gc.h_prep_args.as<PrepareGroupArgs>(); // (its own pinned table: stage C rewrites h_args without waiting)
        for (uint32_t i = 0; i < count; ++i) {
            GroupItem &g = (*pit[i]);
            hp[i].a_raw = g.raw_a;
            hp[i].b_raw = g.raw_b;
            hp[i].n = g.n;
            hp[i].pad = 0;
            hp[i].stats = nullptr;
            hp[i].args = g.fe.prep;
            hp[i].soa = reinterpret_cast<double *>(slot(i, L.pts));
            // (the bound of max|x| comes from the host for the linear cameras; non-linear ones: k_prepare_g leaves it in the slot)
            hp[i].absmax_bits = prefilter_bound_on_device(kind, g.fe.prep) ? reinterpret_cast<unsigned long long *>(slot(i, L.absmax)) : nullptr;
            if (hp[i].absmax_bits) {
                HIP_TRY(hipMemsetAsync(hp[i].absmax_bits, 0, sizeof(unsigned long long), c->stream));
                ++n_dev_absmax;
            }
            // the problem as the kernels see it
            pl_problem &p = g.prob;
            p.kind = kind;
            p.device = c->device;
            p.n = g.n;
            p.d_pts = hp[i].soa;
            p.borrowed = true;
            std::memset(&p.ps, 0, sizeof(p.ps));
            p.ps.n = g.n;
            for (int d = 0; d < nd; ++d)
                p.ps.a[d] = p.d_pts + (size_t)d * g.n;
            p.ps.xy_absmax = g.have_absmax ? g.xy_absmax : group_item_absmax(g); // (a pass over the points: done by the staging hook when there is one)
        }
        HIP_TRY(hipMemcpyAsync(gc.args.p, hp, sizeof(PrepareGroupArgs) * count, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(launch_group_prepare(gc.args.as<PrepareGroupArgs>(), count, max_n, c->stream));
        // (no synchronisation: the device table gc.args is rewritten by a later copy on the same stream, the host table of this
        // stage is not touched again before the group's next synchronisation)
        if (n_dev_absmax) { // ... except for the members whose max|x| only the device knows (as make_problem_prepared reads it back)
            HIP_TRY(gc.h_absmax.ensure(sizeof(unsigned long long) * count));
            for (uint32_t i = 0; i < count; ++i)
                if (hp[i].absmax_bits)
                    HIP_TRY(hipMemcpyAsync(gc.h_absmax.as<unsigned long long>() + i, hp[i].absmax_bits, sizeof(unsigned long long),
                                           hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(wait_stream(c));
            for (uint32_t i = 0; i < count; ++i)
                if (hp[i].absmax_bits) {
                    double amax;
                    std::memcpy(&amax, gc.h_absmax.as<unsigned long long>() + i, sizeof(double));
                    (*pit[i]).prob.ps.xy_absmax = std::nextafter((float)amax, std::numeric_limits<float>::infinity());
                }
        }
    }

    ptA.reset();
    // ---- stage B: one RansacRun per problem ----
    struct Cleanup { // the runs of this call's problems end with it - unless a problem is deferred to a later call
        GroupItem *const *pit;
        uint32_t count;
        ~Cleanup() {
            for (uint32_t i = 0; i < count; ++i)
                if (!pit[i]->deferred) {
                    delete pit[i]->run;
                    pit[i]->run = nullptr;
                }
        }
    } cleanup{pit, count};
    std::vector<uint32_t> warm_members;
    for (uint32_t i = 0; i < count; ++i) {
        GroupItem &g = (*pit[i]);
        if (resume && g.run) { // a deferred problem: the sequential loop's state lives on, on this worker's stream now
            g.run->c = c;
            g.deferred = false;
            g.active = true;
            continue;
        }
        g.t_start = now_s();
        const bool warm = g.fe.scaled.ransac.score_initial_model != 0;
        if (!resident)
            front_initial_record(g.fe, g.item->model, g.rec);
        else if (warm) // (a resident problem's model is in the problem's coordinates already)
            record_from_model(kind, g.ritem->model, g.rec);
        else
            identity_record(kind, g.rec);
        g.run = new RansacRun(c, &g.prob, &g.fe.scaled, g.rec, nullptr, g.st);
        g.run->MAXM = (int)maxm;
        std::memset(g.st, 0, sizeof(*g.st));
        g.st->model_score = std::numeric_limits<double>::max();
        g.looped = g.n >= (uint32_t)K;
        g.active = g.looped && !g.fallback;
        if (g.active) {
            g.st->num_inliers = 0;
            if (warm)
                warm_members.push_back(i); // (scored and refined together below, then begin_loop)
            else
                g.run->begin_loop();
        }
    }

    // Every local optimisation the members have queued (RansacRun::jobs) as ONE k_lm launch (tasks in pinned memory), then one
    // re-scoring launch, one synchronisation; the jobs come back with params_out, record_out, count and score.  Used by a batch
    // step (the LOs its improving hypotheses trigger) and by the warm starts in front of the loop.
    auto run_queued_jobs = [&]() -> int {
        uint32_t total_jobs = 0, max_jobs = 0;
        for (uint32_t i = 0; i < count; ++i) {
            GroupItem &g = (*pit[i]);
            if (!g.active)
                continue;
            g.job0 = total_jobs;
            total_jobs += (uint32_t)g.run->jobs.size();
            max_jobs = std::max<uint32_t>(max_jobs, (uint32_t)g.run->jobs.size());
        }
        if (!total_jobs)
            return PL_OK;
        std::unique_ptr<PhaseTimer> ptLm(new PhaseTimer(g_t_lmtasks));
        // every LO of every problem as ONE k_lm launch (tasks in pinned memory), then one re-scoring launch
        const size_t stage_bytes = (sizeof(LMTask) + sizeof(double) * kModelStride) * total_jobs;
        HIP_TRY(gc.h_tasks.ensure(resident ? stage_bytes : raise_hw(g_hw_tasks, stage_bytes)));
        HIP_TRY(gc.lm_records.ensure(sizeof(double) * kModelStride * total_jobs));
        HIP_TRY(gc.lm_scratch.ensure(resident ? (size_t)max_n * total_jobs + 16 : raise_hw(g_hw_lm_scratch, (size_t)max_n * total_jobs + 16)));
        HIP_TRY(gc.seq_count.ensure(sizeof(uint32_t) * total_jobs));
        HIP_TRY(gc.seq_score.ensure(sizeof(double) * total_jobs));
        HIP_TRY(gc.h_count.ensure(sizeof(uint32_t) * total_jobs));
        HIP_TRY(gc.h_score.ensure(sizeof(double) * total_jobs));
        LMTask *ht = gc.h_tasks.as<LMTask>();
        double *hr = reinterpret_cast<double *>(ht + total_jobs);
        LMTask *d_tasks = gc.h_tasks.dev<LMTask>();
        double *d_records_in = reinterpret_cast<double *>(d_tasks + total_jobs);
        SeqScoreArgs *hs = gc.h_args.as<SeqScoreArgs>();
        for (uint32_t i = 0; i < count; ++i) {
            GroupItem &g = (*pit[i]);
            SeqScoreArgs &q = hs[i];
            std::memset(&q, 0, sizeof(q));
            if (!g.active || g.run->jobs.empty())
                continue;
            RansacRun &r = *g.run;
            const uint32_t nj = (uint32_t)r.jobs.size();
            for (uint32_t j = 0; j < nj; ++j) {
                const uint32_t t = g.job0 + j;
                LMTask &T = ht[t];
                std::memset(&T, 0, sizeof(T));
                T.pts = g.prob.ps;
                lm_params_from_record(kind, r.jobs[j].record_in, T.params);
                T.opt = r.jobs[j].opt;
                T.cam = r.jobs[j].cam;
                T.point_scale = r.jobs[j].point_scale;
                T.prefilter_thr2 = r.jobs[j].prefilter_thr2;
                T.mask = nullptr;
                T.scratch = gc.lm_scratch.as<uint8_t>() + (size_t)t * max_n;
                T.record_in = d_records_in + (size_t)t * kModelStride;
                T.record_out = gc.lm_records.as<double>() + (size_t)t * kModelStride;
                std::memcpy(hr + (size_t)t * kModelStride, r.jobs[j].record_in, sizeof(double) * kModelStride);
            }
            q = plain_seq_args(c, g.prob.ps, gc.lm_records.as<double>() + (size_t)g.job0 * kModelStride, nj, r.thr2,
                               gc.seq_count.as<uint32_t>() + g.job0, gc.seq_score.as<double>() + g.job0,
                               gc.h_count.dev<uint32_t>() + g.job0, gc.h_score.dev<double>() + g.job0);
        }
        if (max_jobs >= kIotaEntries)
            return fail(PL_ERR_UNSUPPORTED, "too many local optimisations in one batch of a grouped problem");
        ptLm.reset();
        HIP_TRY(hipMemcpyAsync(gc.args.p, hs, sizeof(SeqScoreArgs) * count, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(launch_lm_tasks(kind, d_tasks, total_jobs, max_n, c->stream));
        HIP_TRY(launch_group_score_seq(kind, gc.args.as<SeqScoreArgs>(), count, max_jobs, c->stream));
        HIP_TRY(wait_stream(c));
        for (uint32_t i = 0; i < count; ++i) {
            GroupItem &g = (*pit[i]);
            if (!g.active)
                continue;
            RansacRun &r = *g.run;
            for (uint32_t j = 0; j < (uint32_t)r.jobs.size(); ++j) {
                const uint32_t t = g.job0 + j;
                RefineJob &job = r.jobs[j];
                job.skipped = ht[t].skipped != 0;
                std::memcpy(job.params_out, ht[t].params, sizeof(double) * kParamDoubles);
                if (job.skipped)
                    std::memcpy(job.record_out, job.record_in, sizeof(double) * kModelStride);
                else
                    record_from_lm_params(kind, ht[t].params, job.record_out);
                job.count = gc.h_count.as<uint32_t>()[t];
                job.score = gc.h_score.as<double>()[t];
            }
        }
        return PL_OK;
    };

    // ---- the warm starts of the group (ransac.score_initial_model; ransac_impl.h:171-176 = RansacRun::score_initial_model of the
    // single-problem path, for all warm-started members at once): one launch scores every initial model in the reference's summation
    // order, the models that beat the empty record are refined by one k_lm launch and re-scored - two synchronisations for the group
    // instead of two per member (round 6, first form: an all-warm-start batch 27 k problems/s) ----
    if (!warm_members.empty()) {
        const uint32_t nw = (uint32_t)warm_members.size();
        HIP_TRY(gc.h_tasks.ensure(resident ? sizeof(double) * kModelStride * nw : raise_hw(g_hw_tasks, sizeof(double) * kModelStride * nw)));
        HIP_TRY(gc.lm_records.ensure(sizeof(double) * kModelStride * nw));
        HIP_TRY(gc.seq_count.ensure(sizeof(uint32_t) * nw));
        HIP_TRY(gc.seq_score.ensure(sizeof(double) * nw));
        HIP_TRY(gc.h_count.ensure(sizeof(uint32_t) * nw));
        HIP_TRY(gc.h_score.ensure(sizeof(double) * nw));
        double *hrec = gc.h_tasks.as<double>();
        SeqScoreArgs *hs = gc.h_args.as<SeqScoreArgs>();
        for (uint32_t i = 0; i < count; ++i)
            std::memset(&hs[i], 0, sizeof(SeqScoreArgs));
        for (uint32_t w = 0; w < nw; ++w) {
            GroupItem &g = (*pit[warm_members[w]]);
            std::memcpy(hrec + (size_t)w * kModelStride, g.rec, sizeof(double) * kModelStride);
            hs[warm_members[w]] = plain_seq_args(c, g.prob.ps, gc.lm_records.as<double>() + (size_t)w * kModelStride, 1, g.run->thr2,
                                                 gc.seq_count.as<uint32_t>() + w, gc.seq_score.as<double>() + w,
                                                 gc.h_count.dev<uint32_t>() + w, gc.h_score.dev<double>() + w);
        }
        HIP_TRY(hipMemcpyAsync(gc.lm_records.p, hrec, sizeof(double) * kModelStride * nw, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(gc.args.p, hs, sizeof(SeqScoreArgs) * count, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(launch_group_score_seq(kind, gc.args.as<SeqScoreArgs>(), count, 1, c->stream));
        HIP_TRY(wait_stream(c));
        std::vector<uint32_t> cnts(nw);
        std::vector<double> scs(nw);
        for (uint32_t w = 0; w < nw; ++w) // (the LM phase below reuses these pinned arrays)
            cnts[w] = gc.h_count.as<uint32_t>()[w], scs[w] = gc.h_score.as<double>()[w];
        for (uint32_t i = 0; i < count; ++i)
            if ((*pit[i]).run)
                (*pit[i]).run->jobs.clear();
        for (uint32_t w = 0; w < nw; ++w) {
            RansacRun &r = *(*pit[warm_members[w]]).run;
            const uint64_t cnt = cnts[w];
            const double sc = scs[w];
            const bool more = cnt > r.best_min_inl, better = sc < r.best_min_score;
            if (!(more || better))
                continue;
            if (more)
                r.best_min_inl = cnt;
            if (better)
                r.best_min_score = sc;
            if (sc < r.st->model_score) {
                r.st->model_score = sc;
                r.st->num_inliers = cnt;
            }
            r.jobs.push_back(r.make_lo_job(r.best_record));
        }
        {
            const int rc_jobs = run_queued_jobs();
            if (rc_jobs != PL_OK)
                return rc_jobs;
        }
        for (uint32_t w = 0; w < nw; ++w) {
            RansacRun &r = *(*pit[warm_members[w]]).run;
            if (!r.jobs.empty()) {
                const int rc_lo = r.after_lo(r.jobs[0]);
                if (rc_lo != PL_OK)
                    return rc_lo;
            }
            r.jobs.clear();
            r.begin_loop();
        }
    }

    // ---- stage C: batch steps in lock-step ----
    std::vector<size_t> hexp_of; // expected hypotheses of each member's batch of the step
    for (uint32_t step = 0;; ++step) {
        if (max_steps && step >= max_steps) { // the long runs of the group continue in a later, regrouped call
            for (uint32_t i = 0; i < count; ++i) {
                GroupItem &g = (*pit[i]);
                if (g.active && !g.run->stopped && g.run->it < g.run->ro.max_iterations && !(g.run->it > g.run->ro.min_iterations && g.run->it > g.run->dyn_max))
                    g.deferred = true, g.active = false;
            }
            break;
        }
        std::unique_ptr<PhaseTimer> ptArgs(new PhaseTimer(g_t_args));
        GroupArgs *ha = gc.h_args.as<GroupArgs>();
        GroupDims dims;
        std::memset(&dims, 0, sizeof(dims));
        dims.G = count;
        dims.P = P;
        dims.min_n = 0xffffffffu;
        uint32_t nactive = 0;
        std::vector<uint32_t> prosac_members;
        hexp_of.assign(count, 0);
        for (uint32_t i = 0; i < count; ++i) {
            GroupItem &g = (*pit[i]);
            GroupArgs &a = ha[i];
            std::memset(&a, 0, sizeof(a));
            if (!g.active)
                continue;
            RansacRun &r = *g.run;
            if (!r.plan_batch(g.b)) {
                g.active = false;
                continue;
            }
            if (resume) // a regrouped long run: everything the loop is known to need at least, in one batch (plan_batch's doubling
                        // bounds the waste of a single problem's run; here the step overhead of the group is what counts)
                g.b.B = g.b.hi_g = g.b.Bl = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(g.b.B, r.needed_now()), 32768);
            else if (step > 0) // round 6: from the second step on a member asks for what its loop is known to need (the stop
                               // rule's bound after the first local optimisations) instead of doubling - a step of the group is
                               // ~1 ms of chain whatever its members' batch sizes
                g.b.B = g.b.hi_g = g.b.Bl = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(g.b.B, r.needed_now()), max_B);
            if (g.b.B > max_B) // (a shorter batch, the rest comes with the next step)
                g.b.B = g.b.hi_g = g.b.Bl = max_B;
            const uint32_t B = g.b.B;
            const uint32_t N = g.n;
            const uint64_t M64 = sampler_window(N, K, B);
            if (M64 > max_M || r.pos + M64 >= 0xffffffffull) {
                g.active = false, g.fallback = true;
                continue;
            }
            const BatchRun run = r.batch_run();
            BatchShape s;
            s.B = s.Bl = B, s.lo = 0, s.M = (uint32_t)M64, s.slots = (uint32_t)r.MAXM;
            s.use_mfma = score_uses_mfma(kind, N, run.pf);
            s.chunks = group_member_chunks(kind, s.use_mfma, N);
            s.point_rows = s.chunks * 64u * (uint32_t)P;
            s.prune = score_prune_gate(kind, s.use_mfma, B, s.chunks);
            const BatchBuffers bb = slot_buffers(i);
            wire_batch_step(a, run, s, bb);
            if (r.prosac) { // the member's samples of this step, drawn on the host (sampling.cc:85-136), uploaded below
                g.b.prosac_at_batch_start = r.prosac_sampler;
                prosac_members.push_back(i);
            }
            // hypothesis slices per chunk of correspondences: chosen below, once the launch's active members are known
            // (group_score_slices)
            const uint32_t hcap = a.score.hyp_capacity;
            hexp_of[i] = group_expected_hypotheses(kind, B, hcap);
            // grid extents
            group_dims_sampler(dims, a.samp.M, g.n, B);
            dims.max_hcap = std::max(dims.max_hcap, hcap);
            dims.max_chunks = std::max(dims.max_chunks, a.chunks);
            dims.any_mfma |= a.use_mfma;
            dims.any_queue |= a.use_mfma ? 0u : 1u;
            dims.any_prune |= a.score.prune.st ? 1u : 0u;
            dims.any_bound |= (a.score.prune.st && a.score.prune.bound) ? 1u : 0u;
            ++nactive;
        }
        if (nactive == 0)
            break;
        {
            uint32_t launch_chunks = 0; // of the members k_score_mfma_g serves (the others' workgroups are another kernel's)
            for (uint32_t i = 0; i < count; ++i)
                if (ha[i].active && ha[i].use_mfma)
                    launch_chunks += ha[i].chunks;
            for (uint32_t i = 0; i < count; ++i) {
                GroupArgs &a = ha[i];
                if (!a.active)
                    continue;
                a.slices = group_score_slices(kind, a.use_mfma != 0, hexp_of[i], a.gen.num_iters, a.chunks, launch_chunks);
                dims.max_slices = std::max(dims.max_slices, a.slices);
            }
        }
        if (!prosac_members.empty()) {
            size_t words = 0;
            for (uint32_t i : prosac_members)
                words += (size_t)(*pit[i]).b.B * K;
            HIP_TRY(gc.h_samples.ensure(sizeof(uint32_t) * words));
            uint32_t *hs = gc.h_samples.as<uint32_t>();
            for (uint32_t i : prosac_members) {
                GroupItem &g = (*pit[i]);
                if (!g.active)
                    continue;
                RansacRun &r = *g.run;
                for (uint32_t bb = 0; bb < g.b.B; ++bb)
                    r.prosac_sampler.generate(hs + (size_t)bb * K);
                g.b.pos_after = r.prosac_sampler.pos;
                HIP_TRY(hipMemcpyAsync(slot_buffers(i).samples, hs, sizeof(uint32_t) * (size_t)g.b.B * K, hipMemcpyHostToDevice, c->stream));
                hs += (size_t)g.b.B * K;
            }
        }
        ptArgs.reset();
        HIP_TRY(hipMemcpyAsync(gc.args.p, ha, sizeof(GroupArgs) * count, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(launch_group_batch(kind, gc.args.as<GroupArgs>(), dims, c->stream, c->ev0, c->ev1));
        HIP_TRY(wait_stream(c));
        {
            // the scoring launch served `nactive` problems: each books its share (pl_ransac_stats.score_kernel_ms is what
            // bench.py's roofline divides by)
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
            for (uint32_t i = 0; i < count; ++i)
                if ((*pit[i]).active) {
                    (*pit[i]).st->score_kernel_ms += (double)ms / nactive;
                    (*pit[i]).st->score_kernel_launches++;
                }
        }

        // ---- host: improving hypotheses of every problem, the local optimisations they trigger ----
        std::unique_ptr<PhaseTimer> ptImp(new PhaseTimer(g_t_imp));
        for (uint32_t i = 0; i < count; ++i) {
            GroupItem &g = (*pit[i]);
            if (!g.active)
                continue;
            RansacRun &r = *g.run;
            const BatchCtl &hc = gc.h_ctl.as<BatchCtl>()[i];
            if ((hc.orbit_error && !r.prosac) || hc.gen_overflow || hc.num_records > kRecordFirst) {
                g.active = false, g.fallback = true; // (window too small / more than 8 poses / a long candidate list)
                continue;
            }
            if (!r.prosac) // (PROSAC: the host's sampler position, set when the samples were drawn; the device's orbit is not used)
                g.b.pos_after = hc.pos_after;
            g.b.device_positions = !r.prosac;
            g.b.overflow = false;
            g.b.H = g.b.H_local = hc.num_hyp;
            g.b.h_rec = gc.h_recm.as<double>() + (size_t)i * kRecordFirst * kModelStride;
            g.st->nan_hypotheses += hc.nan_hyp;
            const RecordMeta *meta = gc.h_meta.as<RecordMeta>() + (size_t)i * kRecordFirst;
            r.list_improving(meta, hc.num_records, (uint32_t)r.it);
            r.make_jobs(g.b);
        }
        ptImp.reset();
        {
            const int rc_jobs = run_queued_jobs();
            if (rc_jobs != PL_OK)
                return rc_jobs;
        }
        // ---- host: replay of every problem's sequential loop over its batch ----
        PhaseTimer ptReplay(g_t_replay);
        for (uint32_t i = 0; i < count; ++i) {
            GroupItem &g = (*pit[i]);
            if (!g.active)
                continue;
            g.run->defer_offset = true;
            g.run->deferred_offset = -1;
            const int rc = g.run->replay(g.b, nullptr);
            if (rc != PL_OK)
                return rc;
        }
        // hypotheses of the replayed iterations of the problems that stopped inside their batch: offsets[stop] is fetched by
        // stage D's select kernel (a stopped problem's slot is not written again) - no copy and no synchronisation per step
        for (uint32_t i = 0; i < count; ++i) {
            GroupItem &g = (*pit[i]);
            if (g.active && g.run->deferred_offset >= 0) {
                g.off_fetch = g.run->deferred_offset;
                g.run->deferred_offset = -1;
            }
        }
    }

    PhaseTimer ptTail(g_t_tail);
    // Stage E (the front-ends' final bundle on the inliers) is enqueued BEHIND stage D without a synchronisation in between: its tasks
    // take their starting point from the record the select kernel chose and run only if that model has enough inliers (LMTask::
    // start_record / gate_count) - everything else they need is known to the host before stage D.  One wait per group less (of ~6).
    // Not for the fundamental matrix (its starting parameters are an SVD of F on the host) and not for resident problems (no stage E).
    const bool merged_tail = !resident && kind != EST_FUND;
    const uint64_t min_inl = front_min_inliers(kind);
    uint32_t ne = 0, ne_cam = 0; // merged tail: stage E's tasks / those with camera intrinsics
    auto fill_bundle_task = [&](uint32_t i, GroupItem &g, LMTask &T) { // front_bundle over the inliers; abs: on the raw pixels
        const FrontBundle fb = front_bundle(g.fe);
        std::memset(&T, 0, sizeof(T));
        T.pts = g.prob.ps;
        if (kind == EST_ABS) {
            double *soa2 = reinterpret_cast<double *>(slot(i, L.pts2));
            for (int d = 0; d < nd; ++d)
                T.pts.a[d] = soa2 + (size_t)d * g.n;
        }
        T.opt = fb.opt;
        T.cam = fb.cam;
        T.cam_flags = fb.cam_flags;
        T.point_scale = fb.point_scale;
        T.prefilter_thr2 = 0.0;
        T.mask = reinterpret_cast<uint8_t *>(slot(i, L.mask));
        T.scratch = nullptr;
        T.record_in = nullptr;
        T.record_out = nullptr;
    };
    auto fill_prepare2 = [&](uint32_t i, GroupItem &g, PrepareGroupArgs &h) { // the bundle sees the pixels as they are, scaled by 1 / focal
        CameraParams raw_cam;
        std::memset(&raw_cam, 0, sizeof(raw_cam));
        raw_cam.model_id = CAM_NULL;
        h.a_raw = g.raw_a;
        h.b_raw = g.raw_b;
        h.n = g.n;
        h.args = prepare_unproject(raw_cam, nullptr);
        h.soa = reinterpret_cast<double *>(slot(i, L.pts2));
        h.absmax_bits = nullptr;
        h.stats = nullptr;
    };
    // ---- stage D: final refinement of the best model, choice refined / incumbent, inlier mask (ransac_impl.h:190-198;
    // ransac.cc:55, 152, 259, 311) ----
    {
        uint32_t nt = 0;
        for (uint32_t i = 0; i < count; ++i)
            if (!(*pit[i]).fallback && !(*pit[i]).deferred && (*pit[i]).looped)
                (*pit[i]).job0 = nt++;
        const size_t tail_bytes = (sizeof(LMTask) + 2 * sizeof(double) * kModelStride) * std::max<uint32_t>(nt, 1u);
        HIP_TRY(gc.h_tasks.ensure(tail_bytes));
        HIP_TRY(gc.lm_records.ensure(sizeof(double) * kModelStride * std::max<uint32_t>(nt, 1u)));
        HIP_TRY(gc.lm_scratch.ensure((size_t)max_n * std::max<uint32_t>(nt, 1u) + 16));
        HIP_TRY(gc.seq_count.ensure(sizeof(uint32_t) * std::max<uint32_t>(nt, 1u)));
        HIP_TRY(gc.seq_score.ensure(sizeof(double) * std::max<uint32_t>(nt, 1u)));
        HIP_TRY(gc.h_count.ensure(sizeof(uint32_t) * std::max<uint32_t>(nt, 1u)));
        HIP_TRY(gc.h_score.ensure(sizeof(double) * std::max<uint32_t>(nt, 1u)));
        if (merged_tail)
            HIP_TRY(gc.sel_count.ensure(sizeof(uint32_t) * count));
        LMTask *ht = gc.h_tasks.as<LMTask>();
        double *hr = reinterpret_cast<double *>(ht + nt);           // seeds, then the incumbents
        LMTask *d_tasks = gc.h_tasks.dev<LMTask>();
        double *d_rec = reinterpret_cast<double *>(d_tasks + nt);
        // argument tables of the three tail kernels, one block: [SeqScoreArgs x G][SelectArgs x G][MaskArgs x G]
        char *hb = gc.h_args.as<char>();
        SeqScoreArgs *hs = reinterpret_cast<SeqScoreArgs *>(hb);
        SelectArgs *hsel = reinterpret_cast<SelectArgs *>(hb + sizeof(SeqScoreArgs) * count);
        MaskArgs *hm = reinterpret_cast<MaskArgs *>(hb + (sizeof(SeqScoreArgs) + sizeof(SelectArgs)) * count);
        char *db_ = gc.args.as<char>();
        for (uint32_t i = 0; i < count; ++i) {
            GroupItem &g = (*pit[i]);
            std::memset(&hs[i], 0, sizeof(SeqScoreArgs));
            std::memset(&hsel[i], 0, sizeof(SelectArgs));
            std::memset(&hm[i], 0, sizeof(MaskArgs));
            if (g.fallback || g.deferred)
                continue;
            double *d_tmp = reinterpret_cast<double *>(slot(i, L.tmp_model));
            uint8_t *d_mask = reinterpret_cast<uint8_t *>(slot(i, L.mask));
            hm[i].pts = g.prob.ps;
            hm[i].thr2 = g.run->thr2;
            hm[i].mask = d_mask;
            if (g.mdest) // the caller's device memory, written by the mask launch itself: no pinned copy, nothing to copy out below
                hm[i].dst = *g.mdest;
            else
                hm[i].host_mask = gc.h_mask.dev<uint8_t>() + (size_t)g.hmask_slot * max_n;
            if (!g.looped) { // fewer points than the sample (ransac_impl.h:161-163): mask of the untouched model
                // (not reached: group_eligible keeps such problems out; kept for completeness)
                g.fallback = true;
                continue;
            }
            const uint32_t t = g.job0;
            RansacRun &r = *g.run;
            g.st->iterations = r.it;
            const RefineJob job = r.make_lo_job(g.rec);
            LMTask &T = ht[t];
            std::memset(&T, 0, sizeof(T));
            T.pts = g.prob.ps;
            lm_params_from_record(kind, job.record_in, T.params);
            T.opt = job.opt;
            T.cam = job.cam;
            T.point_scale = job.point_scale;
            T.prefilter_thr2 = job.prefilter_thr2;
            T.scratch = gc.lm_scratch.as<uint8_t>() + (size_t)t * max_n;
            T.record_in = d_rec + (size_t)t * kModelStride;
            T.record_out = gc.lm_records.as<double>() + (size_t)t * kModelStride;
            std::memcpy(hr + (size_t)t * kModelStride, g.rec, sizeof(double) * kModelStride);
            std::memcpy(hr + (size_t)(nt + t) * kModelStride, g.rec, sizeof(double) * kModelStride);
            hs[i] = plain_seq_args(c, g.prob.ps, T.record_out, 1, r.thr2, gc.seq_count.as<uint32_t>() + t, gc.seq_score.as<double>() + t,
                                   gc.h_count.dev<uint32_t>() + t, gc.h_score.dev<double>() + t);
            hsel[i].score_refined = hs[i].score;
            hsel[i].incumbent_score = g.st->model_score;
            hsel[i].rec_refined = T.record_out;
            hsel[i].rec_incumbent = d_rec + (size_t)(nt + t) * kModelStride;
            hsel[i].out = d_tmp;
            if (merged_tail) { // the chosen model's inlier count gates the final bundle that is enqueued behind this stage
                hsel[i].count_refined = hs[i].count;
                hsel[i].count_incumbent = (uint32_t)std::min<uint64_t>(g.st->num_inliers, 0xffffffffu);
                hsel[i].count_out = gc.sel_count.as<uint32_t>() + i;
            }
            if (g.off_fetch >= 0) {
                hsel[i].fetch_src = slot_buffers(i).offsets + g.off_fetch;
                hsel[i].fetch_dst = gc.h_offsets.dev<uint32_t>() + i;
            }
            hm[i].model = d_tmp;
        }
        if (nt) {
            HIP_TRY(hipMemcpyAsync(gc.args.p, hb, (sizeof(SeqScoreArgs) + sizeof(SelectArgs) + sizeof(MaskArgs)) * count,
                                   hipMemcpyHostToDevice, c->stream));
            HIP_TRY(launch_lm_tasks(kind, d_tasks, nt, max_n, c->stream));
            HIP_TRY(launch_group_score_seq(kind, reinterpret_cast<SeqScoreArgs *>(db_), count, 1, c->stream));
            HIP_TRY(launch_group_select(reinterpret_cast<SelectArgs *>(db_ + sizeof(SeqScoreArgs) * count), count, c->stream));
            // (slots without a model - fallback - have pts.n = 0 in the table: their blocks return at once)
            HIP_TRY(launch_group_mask(kind, reinterpret_cast<MaskArgs *>(db_ + (sizeof(SeqScoreArgs) + sizeof(SelectArgs)) * count),
                                      count, max_n, c->stream));
            if (merged_tail) { // stage E for every problem of stage D, gated on the device
                for (uint32_t i = 0; i < count; ++i) {
                    GroupItem &g = (*pit[i]);
                    if (g.fallback || g.deferred || !g.looped)
                        continue;
                    ne++;
                    ne_cam += g.fe.cam_flags ? 1u : 0u;
                }
                HIP_TRY(gc.h_tail.ensure(sizeof(LMTask) * std::max<uint32_t>(ne, 1u)));
                LMTask *he = gc.h_tail.as<LMTask>();
                if (kind == EST_ABS) {
                    HIP_TRY(gc.h_prep_args.ensure(sizeof(PrepareGroupArgs) * count));
                    PrepareGroupArgs *hp2 = gc.h_prep_args.as<PrepareGroupArgs>();
                    for (uint32_t i = 0; i < count; ++i) {
                        GroupItem &g = (*pit[i]);
                        std::memset(&hp2[i], 0, sizeof(PrepareGroupArgs));
                        if (!(g.fallback || g.deferred || !g.looped))
                            fill_prepare2(i, g, hp2[i]);
                    }
                    // (gc.args is rewritten by a copy that is stream-ordered behind stage D's kernels)
                    HIP_TRY(hipMemcpyAsync(gc.args.p, hp2, sizeof(PrepareGroupArgs) * count, hipMemcpyHostToDevice, c->stream));
                    HIP_TRY(launch_group_prepare(gc.args.as<PrepareGroupArgs>(), count, max_n, c->stream));
                }
                uint32_t next_plain = 0, next_cam = ne - ne_cam;
                for (uint32_t i = 0; i < count; ++i) {
                    GroupItem &g = (*pit[i]);
                    if (g.fallback || g.deferred || !g.looped)
                        continue;
                    g.job_e = g.fe.cam_flags ? next_cam++ : next_plain++;
                    LMTask &T = he[g.job_e];
                    fill_bundle_task(i, g, T);
                    T.start_record = reinterpret_cast<const double *>(slot(i, L.tmp_model));
                    T.gate_count = gc.sel_count.as<uint32_t>() + i;
                    T.gate_min = (uint32_t)min_inl;
                }
                HIP_TRY(launch_lm_tasks(kind, gc.h_tail.dev<LMTask>(), ne - ne_cam, max_n, c->stream));
                HIP_TRY(launch_lm_cam(gc.h_tail.dev<LMTask>() + (ne - ne_cam), ne_cam, c->stream));
            }
            HIP_TRY(wait_stream(c));
        }
        for (uint32_t i = 0; i < count; ++i) {
            GroupItem &g = (*pit[i]);
            if (g.fallback || g.deferred)
                continue;
            const uint32_t t = g.job0;
            if (g.off_fetch >= 0)
                g.st->hypotheses += gc.h_offsets.as<uint32_t>()[i];
            g.st->refinements++;
            const bool skipped = ht[t].skipped != 0;
            const double sc = gc.h_score.as<double>()[t];
            if (sc < g.st->model_score) {
                if (!skipped)
                    record_from_lm_params(kind, ht[t].params, g.rec);
                g.st->num_inliers = gc.h_count.as<uint32_t>()[t];
            }
            uint8_t *user_mask = resident ? g.ritem->inliers : g.item->inliers;
            if (user_mask && !g.mdest)
                std::memcpy(user_mask, gc.h_mask.as<uint8_t>() + (size_t)g.hmask_slot * max_n, g.n);
            g.st->seconds = now_s() - g.t_start;
        }
    }

    if (resident) { // the ransac_* contract ends here (run_with_model): the model in the user's representation
        for (uint32_t i = 0; i < count; ++i) {
            GroupItem &g = (*pit[i]);
            if (g.fallback || g.deferred)
                continue;
            model_from_record(kind, g.rec, g.ritem->model);
            g.ritem->status = PL_OK;
        }
        return PL_OK;
    }

    // ---- stage E: the front-ends' final refinement on the inliers ----
    if (merged_tail) { // its tasks ran behind stage D: take the results of those the host rule (num_inliers > min) admits
        const LMTask *he = gc.h_tail.as<LMTask>();
        for (uint32_t i = 0; i < count; ++i) {
            GroupItem &g = (*pit[i]);
            if (g.fallback || g.deferred || !g.looped || !ne)
                continue;
            const bool want = g.st->num_inliers > min_inl;
            const bool ran = he[g.job_e].skipped != 2u;
            if (want != ran)
                return fail(PL_ERR_HIP, "merged final bundle: the device gate disagrees with the host rule");
            if (!want)
                continue;
            record_from_lm_params(kind, he[g.job_e].params, g.rec);
            if (g.fe.cam_flags)
                g.cam_refined = he[g.job_e].cam;
        }
    } else { // (the fundamental matrix: resident groups returned above, every other kind took the merged tail)
        uint32_t nt = 0;
        for (uint32_t i = 0; i < count; ++i)
            if (!(*pit[i]).fallback && !(*pit[i]).deferred && (*pit[i]).st->num_inliers > min_inl)
                nt++;
        if (nt) {
            HIP_TRY(gc.h_tasks.ensure(sizeof(LMTask) * nt));
            LMTask *ht = gc.h_tasks.as<LMTask>();
            uint32_t next = 0;
            for (uint32_t i = 0; i < count; ++i) {
                GroupItem &g = (*pit[i]);
                if (g.fallback || g.deferred || !(g.st->num_inliers > min_inl))
                    continue;
                g.job0 = next++;
                fill_bundle_task(i, g, ht[g.job0]);
                lm_params_from_record(kind, g.rec, ht[g.job0].params);
            }
            HIP_TRY(launch_lm_tasks(kind, gc.h_tasks.dev<LMTask>(), nt, max_n, c->stream));
            HIP_TRY(wait_stream(c));
            for (uint32_t i = 0; i < count; ++i) {
                GroupItem &g = (*pit[i]);
                if (g.fallback || g.deferred || !(g.st->num_inliers > min_inl))
                    continue;
                record_from_lm_params(kind, ht[g.job0].params, g.rec); // (final_refine: skipped never happens without a pre-filter)
            }
        }
    }
    // results in the user's representation
    for (uint32_t i = 0; i < count; ++i) {
        GroupItem &g = (*pit[i]);
        if (g.fallback || g.deferred)
            continue;
        pl_batch_item &it = *g.item;
        const bool bundled = g.st->num_inliers > min_inl;
        front_finish(g.fe, g.rec, &g.cam_refined, it.model, kind == EST_ABS && bundled ? it.camera1 : nullptr);
        it.status = PL_OK;
    }
    (void)t_group;
    return PL_OK;
}
