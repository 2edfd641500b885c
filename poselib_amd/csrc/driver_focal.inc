// poselib_amd - host side of the focal-length estimator (included by driver.cc): ransac_pnpf of the reference
// (PoseLib/robust/ransac.cc:58-75 with FocalAbsolutePoseEstimator) on the device.
//
// The loop itself is pl_focal.h's focal_lo_ransac (the same template the CPU tests run against the oracle); this file is its
// device back end: a batch of iterations = k_focal_setup + k_focal_solve + k_focal_score (focal.hip), the local optimisations of a
// batch = one k_lm_cam launch (lm_cam.hip: pose + focal length, truncated loss, 25 iterations - absolute_pose.cc:145-157) followed by
// k_focal_score_wg on the refined models, one round trip.  Everything the loop reads is written by the kernels into one pinned block;
// no copy to or from pageable memory.  One problem = one chain of dispatches on the calling thread's stream (no grouping across
// problems: DESIGN 4 says what that costs under 16 streams).

struct DeviceFocalBackend {
    Context *c;
    const pl_problem *p;
    uint64_t seed;
    double thr2, max_error, max_focal;
    LMOptions lo;

    void fill_points(const double **a) const {
        for (int i = 0; i < 5; ++i)
            a[i] = p->ps.a[i];
    }
    // Every result the host loop reads is written by the kernels themselves into ONE pinned, mapped block (c->h_focal): no copy or
    // fill dispatches, and - what decides the throughput of several host threads - no copies to or from pageable memory, each of
    // which pins and unpins its buffer under the process's memory-map lock (round 3's form: 14 such copies per problem; 16 threads
    // reached 2.4 k problems/s, 32 threads less).  Layout for `slots` hypothesis slots of B iterations:
    //   [counts u32 x slots | num_models u32 x B | sums f64 x slots | models FocalModel x slots]
    struct HostOut {
        uint32_t *counts, *num_models;
        double *sums;
        FocalModel *models;
    };
    int host_out(uint32_t slots, uint32_t B, HostOut &h, HostOut &d) {
        const size_t o1 = sizeof(uint32_t) * slots, o2 = o1 + sizeof(uint32_t) * B;
        const size_t o2a = (o2 + 7) & ~(size_t)7, o3 = o2a + sizeof(double) * slots, total = o3 + sizeof(FocalModel) * slots;
        HIP_TRY(c->h_focal.ensure(total));
        auto at = [&](char *base, HostOut &x) {
            x.counts = reinterpret_cast<uint32_t *>(base);
            x.num_models = reinterpret_cast<uint32_t *>(base + o1);
            x.sums = reinterpret_cast<double *>(base + o2a);
            x.models = reinterpret_cast<FocalModel *>(base + o3);
        };
        at(c->h_focal.as<char>(), h);
        at(c->h_focal.dev<char>(), d);
        return PL_OK;
    }
    void fill_score_args(FocalScoreArgs &sa, const HostOut &d, uint32_t slots) const {
        fill_points(sa.a);
        sa.n = p->n;
        sa.models = nullptr;
        sa.num_models = nullptr;
        sa.lm_tasks = nullptr;
        sa.num_slots = slots;
        sa.thr2 = thr2;
        sa.counts = d.counts;
        sa.sums = d.sums;
    }
    int minimal(uint64_t pos_base, const uint32_t *positions, uint32_t B, std::vector<FocalModel> &models,
                std::vector<uint32_t> &num_models, std::vector<uint32_t> &counts, std::vector<double> &sums, const uint32_t *samples = nullptr) {
        const uint32_t slots = B * (uint32_t)kFocalMaxModels;
        // positions, then (PROSAC) the B x kFocalSample explicit sample indices, in one upload
        const size_t words = (size_t)B * (samples ? 1 + kFocalSample : 1);
        HIP_TRY(c->h_positions.ensure(sizeof(uint32_t) * words));
        HIP_TRY(c->models.ensure(sizeof(FocalModel) * slots));
        HIP_TRY(c->num_models.ensure(sizeof(uint32_t) * B));
        HIP_TRY(c->focal_stage.ensure(focal_stage_bytes(B)));
        HostOut h, d;
        int rc = host_out(slots, B, h, d);
        if (rc != PL_OK)
            return rc;
        std::memcpy(c->h_positions.p, positions, sizeof(uint32_t) * B);
        if (samples)
            std::memcpy(c->h_positions.as<uint32_t>() + B, samples, sizeof(uint32_t) * (size_t)B * kFocalSample);
        // (the generator reads the positions / samples from the pinned block itself: no copy dispatch)
        FocalGenArgs ga;
        fill_points(ga.a);
        ga.n = p->n;
        ga.seed = seed;
        ga.pos_base = pos_base;
        ga.positions = c->h_positions.dev<uint32_t>();
        ga.samples = samples ? c->h_positions.dev<uint32_t>() + B : nullptr;
        ga.num_iters = B;
        ga.max_focal = max_focal;
        ga.models = c->models.as<FocalModel>();
        ga.num_models = c->num_models.as<uint32_t>();
        ga.stage = c->focal_stage.as<double>();
        ga.explicit_in = nullptr;
        ga.keep_all = 0;
        ga.host_models = d.models;
        ga.host_num_models = d.num_models;
        HIP_TRY(launch_focal_generate(ga, c->stream));
        FocalScoreArgs sa;
        fill_score_args(sa, d, slots);
        sa.models = ga.models;
        sa.num_models = ga.num_models;
        HIP_TRY(launch_focal_score(sa, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        num_models.assign(h.num_models, h.num_models + B);
        models.clear(), counts.clear(), sums.clear(); // (compact: one entry per model, in (iteration, slot) order)
        for (uint32_t b = 0; b < B; ++b)
            for (uint32_t m = 0; m < num_models[b]; ++m) {
                const size_t s = (size_t)b * kFocalMaxModels + m;
                models.push_back(h.models[s]);
                counts.push_back(h.counts[s]);
                sums.push_back(h.sums[s]);
            }
        return PL_OK;
    }
    int score(const std::vector<FocalModel> &models, std::vector<uint32_t> &counts, std::vector<double> &sums) {
        const uint32_t slots = (uint32_t)models.size();
        counts.clear();
        sums.clear();
        if (slots == 0)
            return PL_OK;
        HostOut h, d;
        int rc = host_out(slots, 0, h, d);
        if (rc != PL_OK)
            return rc;
        std::memcpy(h.models, models.data(), sizeof(FocalModel) * slots); // (the kernel reads the few models from the pinned block)
        FocalScoreArgs sa;
        fill_score_args(sa, d, slots);
        sa.models = d.models;
        HIP_TRY(launch_focal_score(sa, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        counts.assign(h.counts, h.counts + slots);
        sums.assign(h.sums, h.sums + slots);
        return PL_OK;
    }
    int enqueue_refine(const std::vector<FocalModel> &seeds) {
        const uint32_t nj = (uint32_t)seeds.size();
        HIP_TRY(c->h_tasks.ensure(sizeof(LMTask) * nj));
        LMTask *ht = c->h_tasks.as<LMTask>();
        for (uint32_t j = 0; j < nj; ++j) {
            LMTask &t = ht[j];
            std::memset(&t, 0, sizeof(t));
            t.pts = p->ps;
            for (int i = 0; i < 4; ++i)
                t.params[i] = seeds[j].q[i];
            for (int i = 0; i < 3; ++i)
                t.params[4 + i] = seeds[j].t[i];
            t.opt = lo;
            t.cam.model_id = CAM_SIMPLE_PINHOLE;
            t.cam.num_params = 3;
            t.cam.p[0] = seeds[j].f; // {f, 0, 0}
            t.point_scale = 1.0;
            t.cam_flags = CAM_REFINE_FOCAL;
        }
        HIP_TRY(launch_lm_cam(c->h_tasks.dev<LMTask>(), nj, c->stream));
        return PL_OK;
    }
    void collect_refined(std::vector<FocalModel> &refined) {
        const LMTask *ht = c->h_tasks.as<LMTask>();
        for (size_t j = 0; j < refined.size(); ++j) {
            for (int i = 0; i < 4; ++i)
                refined[j].q[i] = ht[j].params[i];
            for (int i = 0; i < 3; ++i)
                refined[j].t[i] = ht[j].params[4 + i];
            refined[j].f = ht[j].cam.p[0];
        }
    }
    int refine(const std::vector<FocalModel> &seeds, std::vector<FocalModel> &refined) {
        refined = seeds;
        if (seeds.empty())
            return PL_OK;
        int rc = enqueue_refine(seeds);
        if (rc != PL_OK)
            return rc;
        HIP_TRY(hipStreamSynchronize(c->stream));
        collect_refined(refined);
        return PL_OK;
    }
    // the local optimisations of a batch and the scores of their results: k_lm_cam, then k_focal_score on the tasks' refined poses -
    // one synchronisation
    int refine_score(const std::vector<FocalModel> &seeds, std::vector<FocalModel> &refined, std::vector<uint32_t> &counts,
                     std::vector<double> &sums) {
        refined = seeds;
        counts.clear();
        sums.clear();
        const uint32_t nj = (uint32_t)seeds.size();
        if (nj == 0)
            return PL_OK;
        int rc = enqueue_refine(seeds);
        if (rc != PL_OK)
            return rc;
        HostOut h, d;
        rc = host_out(nj, 0, h, d);
        if (rc != PL_OK)
            return rc;
        FocalScoreArgs sa;
        fill_score_args(sa, d, nj);
        sa.lm_tasks = c->h_tasks.dev<LMTask>();
        HIP_TRY(launch_focal_score(sa, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        collect_refined(refined);
        counts.assign(h.counts, h.counts + nj);
        sums.assign(h.sums, h.sums + nj);
        return PL_OK;
    }
};

// ransac_pnpf on a resident absolute-pose problem (normalised image points, principal point at the origin).  The device mask of
// the returned model stays in c->mask (the front-end's final bundle reads it).
// host_xy: the caller's image points (n x 2, as it passed them) and host_cam, the camera they are un-projected with (nullptr: they
// are the problem's points as they stand) - compute_max_focal_length walks the image points on the host.
int run_focal(Context *c, const pl_problem *p, const pl_robust_options *o, pl_camera_pose *pose, double *focal, uint8_t *inliers,
              pl_ransac_stats *st, const double *host_xy, const CameraParams *host_cam) {
    if (p->kind != EST_ABS)
        return fail(PL_ERR_INVALID, "the focal-length estimator works on absolute-pose problems");
    const double t_start = now_s();
    std::memset(st, 0, sizeof(*st));
    const uint32_t n = p->n;
    const FocalLoopOptions lo = focal_loop_options(*o, compute_max_focal_length(host_xy, n, host_cam, o->min_fov));
    DeviceFocalBackend be{c, p, o->ransac.seed, o->max_error * o->max_error, o->max_error, lo.max_focal, lo_options(o->max_error)};
    FocalModel best;
    std::memset(&best, 0, sizeof(best));
    best.q[0] = 1.0;
    best.f = 1.0;
    FocalLoopStats fs; // (score_initial_model: the reference scores the identity pose it has just written, ransac.cc:61-66)
    int rc = focal_lo_ransac(be, n, lo, &best, &fs);
    if (rc != PL_OK)
        return rc;
    stats_from_focal_loop(fs, st);
    for (int i = 0; i < 4; ++i)
        pose->q[i] = best.q[i];
    for (int i = 0; i < 3; ++i)
        pose->t[i] = best.t[i];
    *focal = best.f;
    // get_inliers (ransac.cc:72)
    HIP_TRY(c->mask.ensure(std::max<uint32_t>(n, 1u)));
    HIP_TRY(c->h_mask.ensure(std::max<uint32_t>(n, 1u)));
    if (n) {
        HIP_TRY(launch_focal_mask(p->ps.a, n, best, be.thr2, c->mask.as<uint8_t>(), c->h_mask.dev<uint8_t>(), c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (inliers)
            std::memcpy(inliers, c->h_mask.p, n);
    }
    st->seconds = now_s() - t_start;
    return PL_OK;
}
