// poselib_amd - host side of the shared-focal relative pose estimator (included by driver.cc): ransac_shared_focal_relpose of the
// reference (PoseLib/robust/ransac.cc:182-203 with SharedFocalRelativePoseEstimator) and refine_shared_focal_relpose
// (robust/bundle.cc:281-297) on the device.
//
// The loop is pl_focal.h's template with SharedFocalTraits (the same code the CPU tests run against the oracle); this file is its
// device back end: a batch of iterations = k_sfocal_setup + k_sfocal_solve + k_sfocal_score (sfocal.hip), the local optimisations of a
// batch = one k_sfocal_lm launch (pre-filter at 5 thr^2, truncated loss, 25 iterations - relative_pose.cc:173-203) followed by
// k_sfocal_score_wg on the refined models.  Models, counts and scores land in pinned host memory, written by the kernels themselves.
// One problem = one chain of dispatches on the calling thread's stream (no grouping across problems).

struct DeviceSFocalBackend {
    Context *c;
    const pl_problem *p;
    uint64_t seed;
    double thr2;
    LMOptions lo;

    void fill_points(const double **a) const {
        for (int i = 0; i < 4; ++i)
            a[i] = p->ps.a[i];
    }
    // counts and scores go straight into pinned host memory (the kernel writes the slots that hold a model, nothing else is read)
    int score_on_device(const FocalModel *d_models, const uint32_t *d_num_models, uint32_t slots, const SFocalLMTask *d_tasks = nullptr) {
        HIP_TRY(c->h_count.ensure(sizeof(uint32_t) * slots));
        HIP_TRY(c->h_score.ensure(sizeof(double) * slots));
        SFocalScoreArgs sa;
        fill_points(sa.a);
        sa.n = p->n;
        sa.models = d_models;
        sa.num_models = d_num_models;
        sa.lm_tasks = d_tasks;
        sa.num_slots = slots;
        sa.thr2 = thr2;
        sa.counts = c->h_count.dev<uint32_t>();
        sa.scores = c->h_score.dev<double>();
        HIP_TRY(launch_sfocal_score(sa, c->stream));
        return PL_OK;
    }
    int minimal(uint64_t pos_base, const uint32_t *positions, uint32_t B, std::vector<FocalModel> &models,
                std::vector<uint32_t> &num_models, std::vector<uint32_t> &counts, std::vector<double> &scores, const uint32_t *samples = nullptr) {
        const uint32_t slots = B * (uint32_t)kSFocalMaxModels;
        // positions, then (PROSAC) the B x kSFocalSample explicit sample indices, in one upload
        const size_t words = (size_t)B * (samples ? 1 + kSFocalSample : 1);
        HIP_TRY(c->h_positions.ensure(sizeof(uint32_t) * words));
        HIP_TRY(c->models.ensure(sizeof(FocalModel) * slots));
        HIP_TRY(c->num_models.ensure(sizeof(uint32_t) * B));
        HIP_TRY(c->h_models.ensure(sizeof(FocalModel) * slots));
        HIP_TRY(c->h_num_models.ensure(sizeof(uint32_t) * B));
        std::memcpy(c->h_positions.p, positions, sizeof(uint32_t) * B);
        if (samples)
            std::memcpy(c->h_positions.as<uint32_t>() + B, samples, sizeof(uint32_t) * (size_t)B * kSFocalSample);
        // (the generator reads the positions / samples from the pinned block itself: no copy dispatch)
        SFocalGenArgs ga;
        fill_points(ga.a);
        ga.n = p->n;
        ga.seed = seed;
        ga.pos_base = pos_base;
        ga.positions = c->h_positions.dev<uint32_t>();
        ga.samples = samples ? c->h_positions.dev<uint32_t>() + B : nullptr;
        ga.num_iters = B;
        ga.models = c->models.as<FocalModel>();
        ga.num_models = c->num_models.as<uint32_t>();
        // the 0.3 models an iteration yields on average are also written to pinned host memory by the generator itself: no
        // clearing and no copy of the 60 slots per iteration (15.7 MB per batch of 4096 in the first version)
        ga.host_models = c->h_models.dev<FocalModel>();
        ga.host_num_models = c->h_num_models.dev<uint32_t>();
        HIP_TRY(c->focal_stage.ensure(sfocal_stage_bytes(B)));
        ga.stage = c->focal_stage.as<double>();
        ga.explicit_in = nullptr;
        HIP_TRY(launch_sfocal_generate(ga, c->stream));
        int rc = score_on_device(ga.models, ga.num_models, slots);
        if (rc != PL_OK)
            return rc;
        HIP_TRY(hipStreamSynchronize(c->stream));
        num_models.assign(c->h_num_models.as<uint32_t>(), c->h_num_models.as<uint32_t>() + B);
        const FocalModel *hm = c->h_models.as<FocalModel>();
        const uint32_t *hc = c->h_count.as<uint32_t>();
        const double *hs = c->h_score.as<double>();
        models.clear(), counts.clear(), scores.clear(); // (compact: one entry per model, in (iteration, slot) order)
        for (uint32_t b = 0; b < B; ++b)
            for (uint32_t m = 0; m < num_models[b]; ++m) {
                const size_t h = (size_t)b * kSFocalMaxModels + m;
                models.push_back(hm[h]);
                counts.push_back(hc[h]);
                scores.push_back(hs[h]);
            }
        return PL_OK;
    }
    int score(const std::vector<FocalModel> &models, std::vector<uint32_t> &counts, std::vector<double> &scores) {
        const uint32_t slots = (uint32_t)models.size();
        counts.clear();
        scores.clear();
        if (slots == 0)
            return PL_OK;
        HIP_TRY(c->h_models.ensure(sizeof(FocalModel) * slots)); // (the kernel reads the few models from pinned memory: no upload from pageable memory)
        std::memcpy(c->h_models.p, models.data(), sizeof(FocalModel) * slots);
        int rc = score_on_device(c->h_models.dev<FocalModel>(), nullptr, slots);
        if (rc != PL_OK)
            return rc;
        HIP_TRY(hipStreamSynchronize(c->stream));
        counts.assign(c->h_count.as<uint32_t>(), c->h_count.as<uint32_t>() + slots);
        scores.assign(c->h_score.as<double>(), c->h_score.as<double>() + slots);
        return PL_OK;
    }
    // tasks of `count` refinements in pinned memory; prefilter: the estimator's refine_model, otherwise `mask` (may be null)
    int enqueue_lm(const FocalModel *seeds, uint32_t nj, const LMOptions &opt, double prefilter_thr2, const uint8_t *mask) {
        const size_t npad = ((size_t)p->n + 255u) & ~(size_t)255u;
        HIP_TRY(c->h_tasks.ensure(sizeof(SFocalLMTask) * nj));
        if (prefilter_thr2 > 0)
            HIP_TRY(c->lm_scratch.ensure(npad * nj));
        SFocalLMTask *ht = c->h_tasks.as<SFocalLMTask>();
        for (uint32_t j = 0; j < nj; ++j) {
            SFocalLMTask &t = ht[j];
            std::memset(&t, 0, sizeof(t));
            fill_points(t.a);
            t.n = p->n;
            for (int i = 0; i < 4; ++i)
                t.params[i] = seeds[j].q[i];
            for (int i = 0; i < 3; ++i)
                t.params[4 + i] = seeds[j].t[i];
            t.params[kSFocalFocalSlot] = seeds[j].f;
            t.opt = opt;
            t.prefilter_thr2 = prefilter_thr2;
            t.mask = mask;
            t.scratch = prefilter_thr2 > 0 ? c->lm_scratch.as<uint8_t>() + npad * j : nullptr;
        }
        HIP_TRY(launch_sfocal_lm(c->h_tasks.dev<SFocalLMTask>(), nj, c->stream));
        return PL_OK;
    }
    void collect_lm(const FocalModel *seeds, uint32_t nj, FocalModel *out, SFocalLMTask *first_task_out) const {
        const SFocalLMTask *ht = c->h_tasks.as<SFocalLMTask>();
        for (uint32_t j = 0; j < nj; ++j) {
            out[j] = seeds[j];
            if (ht[j].skipped)
                continue; // (<= 6 approximate inliers: refine_model returns without touching the model)
            for (int i = 0; i < 4; ++i)
                out[j].q[i] = ht[j].params[i];
            for (int i = 0; i < 3; ++i)
                out[j].t[i] = ht[j].params[4 + i];
            out[j].f = ht[j].params[kSFocalFocalSlot];
        }
        if (first_task_out)
            *first_task_out = ht[0];
    }
    int run_lm(const FocalModel *seeds, uint32_t nj, const LMOptions &opt, double prefilter_thr2, const uint8_t *mask, FocalModel *out,
               SFocalLMTask *first_task_out = nullptr) {
        if (nj == 0)
            return PL_OK;
        int rc = enqueue_lm(seeds, nj, opt, prefilter_thr2, mask);
        if (rc != PL_OK)
            return rc;
        HIP_TRY(hipStreamSynchronize(c->stream));
        collect_lm(seeds, nj, out, first_task_out);
        return PL_OK;
    }
    // the local optimisations of a batch and the scores of their results: k_sfocal_lm, then k_sfocal_score_wg on the models the tasks
    // hold afterwards - one synchronisation (round 5; two before: refine, read back, score)
    int refine_score(const std::vector<FocalModel> &seeds, std::vector<FocalModel> &refined, std::vector<uint32_t> &counts,
                     std::vector<double> &scores) {
        refined = seeds;
        counts.clear();
        scores.clear();
        const uint32_t nj = (uint32_t)seeds.size();
        if (nj == 0)
            return PL_OK;
        int rc = enqueue_lm(seeds.data(), nj, lo, 5 * thr2, nullptr);
        if (rc != PL_OK)
            return rc;
        rc = score_on_device(nullptr, nullptr, nj, c->h_tasks.dev<SFocalLMTask>());
        if (rc != PL_OK)
            return rc;
        HIP_TRY(hipStreamSynchronize(c->stream));
        collect_lm(seeds.data(), nj, refined.data(), nullptr);
        counts.assign(c->h_count.as<uint32_t>(), c->h_count.as<uint32_t>() + nj);
        scores.assign(c->h_score.as<double>(), c->h_score.as<double>() + nj);
        return PL_OK;
    }
    int refine(const std::vector<FocalModel> &seeds, std::vector<FocalModel> &refined) {
        refined = seeds;
        return run_lm(seeds.data(), (uint32_t)seeds.size(), lo, 5 * thr2, nullptr, refined.data());
    }
};

// ransac_shared_focal_relpose on a resident two-view problem (points relative to the principal point).  pose / focal: the initial
// model when score_initial_model is set, the result on return.  The device mask of the returned model stays in c->mask.
int run_shared_focal(Context *c, const pl_problem *p, const pl_robust_options *o, pl_camera_pose *pose, double *focal, uint8_t *inliers,
                     pl_ransac_stats *st) {
    if (p->kind == EST_ABS)
        return fail(PL_ERR_INVALID, "the shared-focal estimator works on two-view problems");
    const double t_start = now_s();
    std::memset(st, 0, sizeof(*st));
    const uint32_t n = p->n;
    const FocalLoopOptions lo = focal_loop_options(*o, -1.0);
    DeviceSFocalBackend be{c, p, o->ransac.seed, o->max_error * o->max_error, lo_options(o->max_error)};
    FocalModel best;
    std::memset(&best, 0, sizeof(best));
    if (lo.score_initial_model) {
        for (int i = 0; i < 4; ++i)
            best.q[i] = pose->q[i];
        for (int i = 0; i < 3; ++i)
            best.t[i] = pose->t[i];
        best.f = *focal;
    } else { // ransac.cc:185-190
        best.q[0] = 1.0;
        best.f = 1.0;
    }
    FocalLoopStats fs;
    int rc = focal_lo_ransac_t<SharedFocalTraits>(be, n, lo, &best, &fs);
    if (rc != PL_OK)
        return rc;
    stats_from_focal_loop(fs, st);
    for (int i = 0; i < 4; ++i)
        pose->q[i] = best.q[i];
    for (int i = 0; i < 3; ++i)
        pose->t[i] = best.t[i];
    *focal = best.f;
    // get_inliers(F, ...) (ransac.cc:194-200)
    // (g_mask_dest, pl_estimate_shared_focal_relative_pose_dev with a device mask: the launch writes the caller's device memory
    // itself - no pinned copy, `inliers` is ignored)
    const MaskDest *dst = g_mask_dest;
    HIP_TRY(c->mask.ensure(std::max<uint32_t>(n, 1u)));
    if (!dst)
        HIP_TRY(c->h_mask.ensure(std::max<uint32_t>(n, 1u)));
    if (n) {
        HIP_TRY(launch_sfocal_mask(p->ps.a, n, best, be.thr2, c->mask.as<uint8_t>(), dst ? nullptr : c->h_mask.dev<uint8_t>(), c->stream, dst));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (inliers && !dst)
            std::memcpy(inliers, c->h_mask.p, n);
    }
    st->seconds = now_s() - t_start;
    return PL_OK;
}

// refine_shared_focal_relpose (bundle.cc:281-297) on the correspondences of p selected by the device mask (null: all of them)
int refine_shared_focal(Context *c, const pl_problem *p, const LMOptions &opt, const uint8_t *d_mask, pl_camera_pose *pose, double *focal,
                        uint32_t *lm_iterations) {
    DeviceSFocalBackend be{c, p, 0, 0.0, opt};
    FocalModel seed, out;
    for (int i = 0; i < 4; ++i)
        seed.q[i] = pose->q[i];
    for (int i = 0; i < 3; ++i)
        seed.t[i] = pose->t[i];
    seed.f = *focal;
    SFocalLMTask t;
    int rc = be.run_lm(&seed, 1, opt, 0.0, d_mask, &out, &t);
    if (rc != PL_OK)
        return rc;
    for (int i = 0; i < 4; ++i)
        pose->q[i] = out.q[i];
    for (int i = 0; i < 3; ++i)
        pose->t[i] = out.t[i];
    *focal = out.f;
    if (lm_iterations)
        *lm_iterations = t.iterations;
    return PL_OK;
}

// robust.cc:377-386: the image points relative to the principal point, then normalize_points(scale only, shared): the order-dependent
// reduction (mean distance) summed here like the reference, the per-point part (subtract, divide) applied by k_prepare
// the mean distance from the sum of 2 n distances.  One out-of-line function for the host form and the device form's call without
// rows (n == 0: 0.0 / 0.0), so that both get the quotient - its NaN's sign bit included - from the same instruction
__attribute__((noinline)) double mean_distance_scale(double sum, size_t n) { return sum / (std::sqrt(2) * n); }
// (the per-point part, for a scale that is already known: the device form reads it back from k_point_stats)
void prepare_about(double ppx, double ppy, double scale, PrepareArgs &pa) {
    std::memset(&pa, 0, sizeof(pa));
    pa.mode = 2;
    pa.centred = 1;
    pa.c1x = ppx, pa.c1y = ppy, pa.c2x = ppx, pa.c2y = ppy;
    pa.scale = scale;
}
double normalization_about(const double *x1, const double *x2, size_t n, double ppx, double ppy, PrepareArgs &pa) {
    double scale = 0.0;
    for (size_t k = 0; k < n; ++k) {
        const double a0 = x1[2 * k] - ppx, a1 = x1[2 * k + 1] - ppy, b0 = x2[2 * k] - ppx, b1 = x2[2 * k + 1] - ppy;
        scale += std::sqrt(a0 * a0 + a1 * a1);
        scale += std::sqrt(b0 * b0 + b1 * b1);
    }
    scale = mean_distance_scale(scale, n);
    prepare_about(ppx, ppy, scale, pa);
    return scale;
}
