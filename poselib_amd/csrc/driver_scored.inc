// poselib_amd — device-resident matches with their confidences (pl_device_scores): the ranking in front of the *_dev entry points.
// Included by driver.cc inside extern "C", behind driver_dev.inc; the batched form is in driver_batch.inc.
//
// A scored item becomes a plain one before anything of the existing path sees it:
//   rank_sequence (rank.hip)   the permutation of the kept rows and their count, in device memory
//   k_ingest_ranked            the caller's rows order[j] -> row j of contiguous fp64 blocks (Context::ranked_pts, n rows of room:
//                              the launch follows the ranking on the stream and reads the count on the device)
//   one synchronisation        the counts (the kernels write them into pinned memory) and the permutations come back
// and the matching pl_estimate_*_dev runs on those blocks with n = n_used - contiguous fp64, so it reads them where they lie and
// every check, every small-n answer and every refusal is that entry point's own.  Its mask (n_used bytes) is scattered into the
// caller's numbering on the host, with the permutation that came back.
namespace {

int run_item_dev(const pl_batch_item_dev &it, const MaskDest *mdest = nullptr); // (driver_batch.inc: the matching pl_estimate_*_dev)

int check_scores_plain(const pl_device_scores *d, size_t n) {
    if (!d)
        return fail(PL_ERR_INVALID, "device scores: descriptor is null");
    if (n > 0x7fffffffu)
        return fail(PL_ERR_INVALID, "too many correspondences");
    if (d->dtype != PL_F64 && d->dtype != PL_F32)
        return fail(PL_ERR_INVALID, "device scores: dtype must be PL_F64 or PL_F32");
    if (d->stride < 1)
        return fail(PL_ERR_INVALID, "device scores: stride (elements) is below 1");
    if (d->stride > ((int64_t)1 << 28))
        return fail(PL_ERR_INVALID, "device scores: stride beyond 2^28 elements");
    if (!d->data && n)
        return fail(PL_ERR_INVALID, "device scores: data is null");
    const uintptr_t elt = d->dtype == PL_F32 ? sizeof(float) : sizeof(double);
    if (reinterpret_cast<uintptr_t>(d->data) % elt)
        return fail(PL_ERR_INVALID, "device scores: data is not aligned to its element size");
    if (d->min_score != d->min_score)
        return fail(PL_ERR_INVALID, "device scores: min_score is NaN");
    return PL_OK;
}
// the scores as a one-column point set: the memory checks are those of the points, the message names the scores
pl_device_points scores_as_points(const pl_device_scores *d) {
    pl_device_points p;
    p.data = d->data, p.row_stride = d->stride, p.dtype = d->dtype, p.cols = 1;
    return p;
}
int name_the_scores(int rc) {
    if (rc != PL_OK) {
        const size_t at = g_err.find("device points");
        if (at != std::string::npos)
            g_err.replace(at, 13, "device scores");
    }
    return rc;
}
int check_scores_device(const Context *c, const pl_device_scores *d, size_t n) {
    const pl_device_points p = scores_as_points(d);
    return name_the_scores(check_points_device(c, &p, n));
}

RankSrc rank_src(const pl_device_scores *d) {
    RankSrc s;
    s.data = d->data, s.stride = d->stride, s.f32 = d->dtype == PL_F32, s.pad = 0, s.min_score = d->min_score;
    return s;
}

// The members of one ranking: where each one's permutation lies in Context::rank_order and, with `ingest`, its blocks in
// Context::ranked_pts.  Everything is enqueued on the context's stream; Ranking::run waits once and leaves the counts and the
// permutations in host memory.
struct RankMember {
    const pl_device_scores *scores;
    size_t n;
    const pl_device_points *a = nullptr, *b = nullptr; // with both: the permuted copy follows the ranking
    size_t order_at = 0;                               // (out) first slot of the member in the order block
    double *out_a = nullptr, *out_b = nullptr;         // (out) its fp64 blocks, n rows of room each
    size_t kept = 0;                                   // (out, after the wait)
};
struct Ranking {
    const uint32_t *order = nullptr; // all members' slots, member after member (Context::h_rank_order: pinned - the permutations of a
                                     // large batch are tens of megabytes, and a copy into pageable memory took longer than the ranking)
    int run(Context *c, std::vector<RankMember> &m, bool grouped) {
        const size_t count = m.size();
        if (count == 0)
            return PL_OK;
        size_t slots = 0, merge_rows = 0, doubles = 0;
        uint32_t max_n = 0;
        bool ingest = false;
        for (RankMember &r : m)
            max_n = std::max(max_n, (uint32_t)r.n);
        const uint32_t tile = rank_tile(max_n);
        for (RankMember &r : m) {
            r.order_at = slots;
            slots += r.n;
            if (r.n > tile)
                merge_rows += r.n;
            if (r.a && r.b)
                doubles += (size_t)(r.a->cols + r.b->cols) * r.n, ingest = true;
        }
        HIP_TRY(c->rank_order.ensure(sizeof(uint32_t) * std::max<size_t>(slots, 1)));
        if (merge_rows) {
            HIP_TRY(c->rank_keys.ensure(sizeof(unsigned long long) * 2 * merge_rows));
            HIP_TRY(c->rank_rows.ensure(sizeof(uint32_t) * 2 * merge_rows));
        }
        if (ingest)
            HIP_TRY(c->ranked_pts.ensure(sizeof(double) * std::max<size_t>(doubles, 1)));
        // pinned: the counts, then the two tables
        const size_t counts_bytes = (sizeof(uint32_t) * count + 15) & ~(size_t)15;
        HIP_TRY(c->h_rank.ensure(counts_bytes + (sizeof(RankArgs) + sizeof(IngestRankedArgs)) * count));
        uint32_t *kept = c->h_rank.as<uint32_t>();
        RankArgs *ra = reinterpret_cast<RankArgs *>(c->h_rank.as<char>() + counts_bytes);
        IngestRankedArgs *ia = reinterpret_cast<IngestRankedArgs *>(ra + count);
        uint32_t *d_kept = c->h_rank.dev<uint32_t>();
        RankArgs *d_ra = reinterpret_cast<RankArgs *>(c->h_rank.dev<char>() + counts_bytes);
        IngestRankedArgs *d_ia = reinterpret_cast<IngestRankedArgs *>(d_ra + count);
        size_t merge_at = 0, doubles_at = 0;
        for (size_t k = 0; k < count; ++k) {
            RankMember &r = m[k];
            kept[k] = 0;
            std::memset(&ra[k], 0, sizeof(ra[k]));
            std::memset(&ia[k], 0, sizeof(ia[k]));
            ra[k].s = rank_src(r.scores);
            ra[k].n = (uint32_t)r.n;
            if (r.n > tile) {
                ra[k].keys[0] = c->rank_keys.as<unsigned long long>() + 2 * merge_at, ra[k].keys[1] = ra[k].keys[0] + r.n;
                ra[k].rows[0] = c->rank_rows.as<uint32_t>() + 2 * merge_at, ra[k].rows[1] = ra[k].rows[0] + r.n;
                merge_at += r.n;
            }
            ra[k].order = c->rank_order.as<uint32_t>() + r.order_at;
            ra[k].kept = d_kept + k;
            if (r.a && r.b && r.n) {
                r.out_a = c->ranked_pts.as<double>() + doubles_at, doubles_at += (size_t)r.a->cols * r.n;
                r.out_b = c->ranked_pts.as<double>() + doubles_at, doubles_at += (size_t)r.b->cols * r.n;
                ia[k].a = ingest_src(r.a), ia[k].b = ingest_src(r.b);
                ia[k].n = (uint32_t)r.n;
                ia[k].order = ra[k].order, ia[k].kept = ra[k].kept;
                ia[k].out_a = r.out_a, ia[k].out_b = r.out_b;
            }
        }
        if (grouped) {
            HIP_TRY(launch_rank_g(d_ra, (uint32_t)count, max_n, c->stream));
            if (ingest)
                HIP_TRY(launch_ingest_ranked_g(d_ia, (uint32_t)count, max_n, c->stream));
        } else {
            for (size_t k = 0; k < count; ++k) {
                HIP_TRY(launch_rank(ra[k], c->stream));
                if (ia[k].n)
                    HIP_TRY(launch_ingest_ranked(ia[k], c->stream));
            }
        }
        HIP_TRY(c->h_rank_order.ensure(sizeof(uint32_t) * std::max<size_t>(slots, 1)));
        order = c->h_rank_order.as<uint32_t>();
        if (slots)
            HIP_TRY(hipMemcpyAsync(c->h_rank_order.p, c->rank_order.p, sizeof(uint32_t) * slots, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(wait_stream(c));
        for (size_t k = 0; k < count; ++k) {
            if (kept[k] > m[k].n)
                return fail(PL_ERR_HIP, "ranking of the scores: a kept count beyond the member's rows");
            m[k].kept = kept[k];
        }
        return PL_OK;
    }
    // a mask over the kept rows -> the caller's numbering
    void scatter(const RankMember &r, const uint8_t *ranked_mask, uint8_t *inliers) const {
        std::memset(inliers, 0, r.n);
        for (size_t j = 0; j < r.kept; ++j)
            inliers[order[r.order_at + j]] = ranked_mask[j];
    }
};

// a member's permuted blocks as the point sets of a plain item
pl_device_points ranked_points(const double *data, int cols, size_t kept) {
    pl_device_points p;
    p.data = kept ? data : nullptr, p.row_stride = cols, p.dtype = PL_F64, p.cols = cols;
    return p;
}

} // namespace

int pl_debug_rank_tile(size_t max_n) { return (int)rank_tile((uint32_t)std::min<size_t>(max_n, 0x7fffffffu)); }

int pl_debug_rank_scores(const pl_device_scores *scores, const size_t *n, size_t count, uint32_t *order, size_t *kept) {
    if (!scores || !n || !order || !kept)
        return fail(PL_ERR_INVALID, "a pointer is null");
    if (count == 0)
        return PL_OK;
    int rc = PL_OK;
    for (size_t k = 0; k < count && rc == PL_OK; ++k)
        rc = check_scores_plain(&scores[k], n[k]);
    Context *c = nullptr;
    if (rc == PL_OK)
        rc = get_context(&c);
    DeviceAllocationCache allocations;
    for (size_t k = 0; k < count && rc == PL_OK; ++k) {
        const pl_device_points p = scores_as_points(&scores[k]);
        rc = name_the_scores(allocations.check(c, &p, n[k]));
    }
    if (rc != PL_OK)
        return rc;
    std::vector<RankMember> m(count);
    for (size_t k = 0; k < count; ++k)
        m[k].scores = &scores[k], m[k].n = n[k];
    Ranking ranking;
    rc = ranking.run(c, m, /*grouped=*/count > 1);
    if (rc != PL_OK)
        return rc;
    for (size_t k = 0; k < count; ++k) {
        kept[k] = m[k].kept;
        std::memcpy(order + m[k].order_at, ranking.order + m[k].order_at, sizeof(uint32_t) * m[k].kept);
    }
    return PL_OK;
}

int pl_estimate_dev_scored(int kind, const pl_device_points *a, const pl_device_points *b, const pl_device_scores *scores, size_t n,
                           const pl_robust_options *opt, pl_camera *camera1, const pl_camera *camera2, void *model, uint8_t *inliers,
                           pl_ransac_stats *stats, size_t *n_used) {
    if (n_used)
        *n_used = 0;
    if (kind < 0 || kind > 3)
        return fail(PL_ERR_INVALID, "pl_estimate_dev_scored: kind must be 0..3");
    int rc = dev_entry_precheck(kind, opt, camera1, camera2); // what the plain entry point says before it looks at the points
    if (rc == PL_OK)
        rc = check_points_plain(a, n, 2);
    if (rc == PL_OK)
        rc = check_points_plain(b, n, kind == EST_ABS ? 3 : 2);
    if (rc == PL_OK)
        rc = check_scores_plain(scores, n);
    Context *c = nullptr;
    if (rc == PL_OK)
        rc = get_context(&c);
    if (rc == PL_OK)
        rc = check_points_device(c, a, n);
    if (rc == PL_OK)
        rc = check_points_device(c, b, n);
    if (rc == PL_OK)
        rc = check_scores_device(c, scores, n);
    if (rc != PL_OK)
        return rc;
    std::vector<RankMember> m(1);
    m[0].scores = scores, m[0].n = n, m[0].a = a, m[0].b = b;
    Ranking ranking;
    if (n) {
        rc = ranking.run(c, m, /*grouped=*/false);
        if (rc != PL_OK)
            return rc;
    }
    const size_t kept = m[0].kept;
    pl_batch_item_dev it;
    std::memset(&it, 0, sizeof(it));
    it.kind = kind;
    it.a = ranked_points(m[0].out_a, 2, kept), it.b = ranked_points(m[0].out_b, kind == EST_ABS ? 3 : 2, kept);
    it.n = kept;
    it.opt = opt, it.camera1 = camera1, it.camera2 = camera2, it.model = model, it.stats = stats;
    std::vector<uint8_t> ranked_mask(std::max<size_t>(kept, 1), 0);
    it.inliers = inliers ? ranked_mask.data() : nullptr;
    rc = run_item_dev(it);
    if (rc != PL_OK)
        return rc;
    if (inliers)
        ranking.scatter(m[0], ranked_mask.data(), inliers);
    if (n_used)
        *n_used = kept;
    return PL_OK;
}

// The single _dev call - with scores or without - whose inlier mask goes to the caller's device memory.  The destination is
// zero-filled first, on the stream the run follows on; the run's mask launch (RansacRun::run) then writes the flags of its rows
// there itself, a scored item's through the permutation its ranking left in device memory: no pinned host mask, no copy, no
// scatter on the host.  Everything else is pl_estimate_dev_scored / the plain entry point.
int pl_estimate_dev_masked(int kind, const pl_device_points *a, const pl_device_points *b, const pl_device_scores *scores, size_t n,
                           const pl_robust_options *opt, pl_camera *camera1, const pl_camera *camera2, void *model,
                           const pl_device_mask *mask, pl_ransac_stats *stats, size_t *n_used) {
    if (n_used)
        *n_used = 0;
    if (kind < 0 || kind > 3)
        return fail(PL_ERR_INVALID, "pl_estimate_dev_masked: kind must be 0..3");
    int rc = dev_entry_precheck(kind, opt, camera1, camera2); // what the plain entry point says before it looks at the points
    if (rc == PL_OK)
        rc = check_points_plain(a, n, 2);
    if (rc == PL_OK)
        rc = check_points_plain(b, n, kind == EST_ABS ? 3 : 2);
    if (rc == PL_OK && scores)
        rc = check_scores_plain(scores, n);
    if (rc == PL_OK)
        rc = check_mask_plain(mask, n);
    Context *c = nullptr;
    if (rc == PL_OK)
        rc = get_context(&c);
    if (rc == PL_OK)
        rc = check_points_device(c, a, n);
    if (rc == PL_OK)
        rc = check_points_device(c, b, n);
    if (rc == PL_OK && scores)
        rc = check_scores_device(c, scores, n);
    if (rc == PL_OK)
        rc = check_mask_device(c, mask, n);
    if (rc != PL_OK)
        return rc;
    const MaskFillArgs fill = {mask->data, mask->stride, (uint32_t)n, 0};
    rc = enqueue_mask_fill(c, &fill, 1);
    if (rc != PL_OK)
        return rc;
    MaskDest dest = {mask->data, mask->stride, nullptr};
    pl_batch_item_dev it;
    std::memset(&it, 0, sizeof(it));
    it.kind = kind;
    it.a = *a, it.b = *b, it.n = n;
    it.opt = opt, it.camera1 = camera1, it.camera2 = camera2, it.model = model, it.stats = stats;
    if (scores) {
        std::vector<RankMember> m(1);
        m[0].scores = scores, m[0].n = n, m[0].a = a, m[0].b = b;
        Ranking ranking;
        if (n) {
            rc = ranking.run(c, m, /*grouped=*/false);
            if (rc != PL_OK)
                return rc;
        }
        it.a = ranked_points(m[0].out_a, 2, m[0].kept), it.b = ranked_points(m[0].out_b, kind == EST_ABS ? 3 : 2, m[0].kept);
        it.n = m[0].kept;
        dest.order = c->rank_order.as<uint32_t>() + m[0].order_at;
    }
    rc = run_item_dev(it, n ? &dest : nullptr);
    if (rc == PL_OK && n_used)
        *n_used = it.n;
    return rc;
}

// ---------------------------------------------------------------------------- the two estimators of unknown cameras from device memory
// pl_estimate_shared_focal_relative_pose_dev and pl_estimate_1D_radial_absolute_pose_dev: plain, scored and device-mask form of
// each in one entry point.  What their host forms read of the caller's points in front of the loop is one reduction each
// (normalization_about; n / sum |x_k|): k_point_stats makes it over the fp64 rows on the device - the ingested blocks, or the
// permuted blocks a ranking left - in the host's order, one record comes back, and from there the host forms' own code runs
// (shared_focal_run, radial1d_run).  No point passes through the host.
namespace {

// the checks that need no device, then - behind the context - those that ask the runtime; scores and mask may be null
int uncal_check_plain(const pl_device_points *a, int cols_a, const pl_device_points *b, int cols_b, const pl_device_scores *scores,
                      const pl_device_mask *mask, size_t n) {
    int rc = check_points_plain(a, n, cols_a);
    if (rc == PL_OK)
        rc = check_points_plain(b, n, cols_b);
    if (rc == PL_OK && scores)
        rc = check_scores_plain(scores, n);
    if (rc == PL_OK && mask)
        rc = check_mask_plain(mask, n);
    return rc;
}
int uncal_check_device(const Context *c, const pl_device_points *a, const pl_device_points *b, const pl_device_scores *scores,
                       const pl_device_mask *mask, size_t n) {
    int rc = check_points_device(c, a, n);
    if (rc == PL_OK)
        rc = check_points_device(c, b, n);
    if (rc == PL_OK && scores)
        rc = check_scores_device(c, scores, n);
    if (rc == PL_OK && mask)
        rc = check_mask_device(c, mask, n);
    return rc;
}

// The rows a call runs on, as contiguous fp64 blocks behind c->raw_src_a / raw_src_b: with scores the kept rows in ranked order
// (Ranking), otherwise all of them (ingest_points).  A device mask is zero-filled first, on the same stream; its destination -
// through the ranking's permutation for a scored call - is `dest`.
struct UncalRows {
    std::vector<RankMember> m = std::vector<RankMember>(1);
    Ranking ranking;
    size_t used = 0;
    MaskDest dest = {nullptr, 0, nullptr};
    std::vector<uint8_t> ranked_mask; // a scored call's host mask over the kept rows
    bool scored = false;

    int stage(Context *c, const pl_device_points *a, const pl_device_points *b, const pl_device_scores *scores, const pl_device_mask *mask,
              size_t n) {
        scored = scores != nullptr;
        if (mask && n) {
            const MaskFillArgs fill = {mask->data, mask->stride, (uint32_t)n, 0};
            const int rc = enqueue_mask_fill(c, &fill, 1);
            if (rc != PL_OK)
                return rc;
            dest.data = mask->data, dest.stride = mask->stride;
        }
        if (!scores) {
            used = n;
            return ingest_points(c, a, b, n);
        }
        m[0].scores = scores, m[0].n = n, m[0].a = a, m[0].b = b;
        if (n) {
            const int rc = ranking.run(c, m, /*grouped=*/false);
            if (rc != PL_OK)
                return rc;
        }
        used = m[0].kept;
        c->raw_src_a = m[0].out_a, c->raw_src_b = m[0].out_b;
        if (dest.data)
            dest.order = c->rank_order.as<uint32_t>() + m[0].order_at;
        ranked_mask.assign(std::max<size_t>(used, 1), 0);
        return PL_OK;
    }
    const MaskDest *mask_dest() const { return dest.data ? &dest : nullptr; }
    // where the run writes its host mask: nowhere with a device mask, the caller's array, or - scored - the array scatter() reads
    uint8_t *run_mask(uint8_t *inliers) { return dest.data || !inliers ? nullptr : scored ? ranked_mask.data() : inliers; }
    void finish(Context *c, uint8_t *inliers, size_t *n_used) {
        if (scored && inliers && !dest.data)
            ranking.scatter(m[0], ranked_mask.data(), inliers);
        if (n_used)
            *n_used = used;
        c->raw_src_a = c->raw_src_b = nullptr; // (the caller's memory is not read after the call)
    }
};
struct MaskDestScope { // (a run that ends early leaves nothing set for the thread's next call)
    explicit MaskDestScope(const MaskDest *d) { g_mask_dest = d; }
    ~MaskDestScope() { g_mask_dest = nullptr; }
};

// k_point_stats in one of the two modes of unknown cameras over c->raw_src_a / raw_src_b (n > 0)
int uncal_point_stats(Context *c, size_t n, int norm, double cx, double cy, PointStatsRecord *rec) {
    PointStatsArgs args;
    std::memset(&args, 0, sizeof(args));
    args.norm = norm;
    args.cx1 = args.cx2 = cx, args.cy1 = args.cy2 = cy;
    return run_point_stats(c, n, args, rec);
}

} // namespace

int pl_debug_point_stats_about_dev(const pl_device_points *x1, const pl_device_points *x2, size_t n, double cx, double cy, double *out) {
    if (!out)
        return fail(PL_ERR_INVALID, "output pointer is null");
    int rc = check_points_plain(x1, n, 2);
    if (rc == PL_OK && x2)
        rc = check_points_plain(x2, n, 2);
    Context *c = nullptr;
    if (rc == PL_OK)
        rc = get_context(&c);
    if (rc == PL_OK)
        rc = check_points_device(c, x1, n);
    if (rc == PL_OK && x2)
        rc = check_points_device(c, x2, n);
    if (rc != PL_OK)
        return rc;
    out[0] = out[1] = 0.0;
    if (n == 0)
        return PL_OK;
    rc = ingest_points(c, x1, x2, n);
    PointStatsRecord rec;
    if (rc == PL_OK)
        rc = uncal_point_stats(c, n, x2 ? 2 : 3, cx, cy, &rec);
    c->raw_src_a = c->raw_src_b = nullptr;
    if (rc != PL_OK)
        return rc;
    out[0] = rec.scale, out[1] = rec.absmax;
    return PL_OK;
}

namespace {

// The members of one launch of the about-a-centre reduction (k_point_stats_g, norm 2) with the k_ingest_g launch in front of it:
// the stage of pl_estimate_shared_focal_relative_pose_batch_dev's groups and the diagnostic entry below - one piece of code.
struct AboutStatsMember {
    const pl_device_points *a, *b; // N x 2 each, checked
    size_t n;                      // 0: no work, no record
    double cx, cy;
    const double *raw_a = nullptr, *raw_b = nullptr; // (out) the fp64 AoS blocks: a slice of `raw`, or the caller's memory where it is one
};
// Enqueues both launches on the context's stream.  tab (pinned): [records | stats table | ingest table]; raw: room for the sets
// that are not contiguous fp64.  h_rec / d_rec: the records, member after member, as the host and the device address them.
int enqueue_about_stats_g(Context *c, HostBuf &tab, DevBuf &raw, AboutStatsMember *m, uint32_t count, PointStatsRecord **h_rec,
                          PointStatsRecord **d_rec) {
    size_t raw_doubles = 0;
    for (uint32_t i = 0; i < count; ++i)
        raw_doubles += (reads_in_place(m[i].a) ? 0 : 2 * m[i].n) + (reads_in_place(m[i].b) ? 0 : 2 * m[i].n);
    HIP_TRY(raw.ensure(sizeof(double) * std::max<size_t>(raw_doubles, 1)));
    const size_t table_bytes = (sizeof(IngestGroupArgs) + sizeof(PointStatsGroupArgs) + sizeof(PointStatsRecord)) * count;
    HIP_TRY(tab.ensure(table_bytes));
    PointStatsRecord *rec = tab.as<PointStatsRecord>();
    PointStatsGroupArgs *hs = reinterpret_cast<PointStatsGroupArgs *>(rec + count);
    IngestGroupArgs *hi = reinterpret_cast<IngestGroupArgs *>(hs + count);
    *h_rec = rec;
    *d_rec = tab.dev<PointStatsRecord>();
    PointStatsGroupArgs *d_hs = reinterpret_cast<PointStatsGroupArgs *>(*d_rec + count);
    IngestGroupArgs *d_hi = reinterpret_cast<IngestGroupArgs *>(d_hs + count);
    std::memset(rec, 0, table_bytes);
    size_t at = 0;
    uint32_t ingest_n = 0;
    for (uint32_t i = 0; i < count; ++i) {
        AboutStatsMember &r = m[i];
        if (r.n == 0)
            continue;
        double *oa = nullptr, *ob = nullptr;
        if (!reads_in_place(r.a))
            oa = raw.as<double>() + at, at += 2 * r.n;
        if (!reads_in_place(r.b))
            ob = raw.as<double>() + at, at += 2 * r.n;
        if (oa || ob) {
            hi[i].a = ingest_src(r.a), hi[i].b = ingest_src(r.b);
            hi[i].n = (uint32_t)r.n;
            hi[i].out_a = oa, hi[i].out_b = ob;
            ingest_n = std::max(ingest_n, (uint32_t)r.n);
        }
        r.raw_a = oa ? oa : static_cast<const double *>(r.a->data);
        r.raw_b = ob ? ob : static_cast<const double *>(r.b->data);
        hs[i].a_raw = r.raw_a, hs[i].b_raw = r.raw_b;
        hs[i].n = (uint32_t)r.n;
        hs[i].out = *d_rec + i;
        hs[i].args.norm = 2;
        hs[i].args.cx1 = hs[i].args.cx2 = r.cx, hs[i].args.cy1 = hs[i].args.cy2 = r.cy;
        point_stats_sizes(hs[i].args, r.n);
    }
    HIP_TRY(launch_ingest_g(d_hi, count, ingest_n, c->stream));
    HIP_TRY(launch_point_stats_g(d_hs, count, c->stream));
    return PL_OK;
}

int focal_group_stage_device(Context *c, FocalGroupContext &gc, FocalGroupItem *const *pit, uint32_t count) {
    std::vector<AboutStatsMember> m(count);
    for (uint32_t i = 0; i < count; ++i) {
        const FocalGroupItem &g = *pit[i];
        const double *pp = g.item->camera1->params + 1;
        m[i].a = g.src_a, m[i].b = g.src_b, m[i].n = g.n, m[i].cx = pp[0], m[i].cy = pp[1];
    }
    PointStatsRecord *h_rec = nullptr, *d_rec = nullptr;
    const int rc = enqueue_about_stats_g(c, gc.h_dev_tab, gc.raw, m.data(), count, &h_rec, &d_rec);
    if (rc != PL_OK)
        return rc;
    for (uint32_t i = 0; i < count; ++i) {
        FocalGroupItem &g = *pit[i];
        g.raw_a = m[i].raw_a, g.raw_b = m[i].raw_b;
        g.h_rec = h_rec + i, g.d_rec = d_rec + i;
    }
    return PL_OK;
}

// pl_estimate_shared_focal_relative_pose_dev.  ranked_dest: the call is a scored item of the batch form on the blocks its ranking
// left (scores == mask == null) and its mask goes to the caller's device memory through the ranking's permutation
int shared_focal_dev(const pl_device_points *x1, const pl_device_points *x2, const pl_device_scores *scores, size_t n, const double *pp,
                     const pl_robust_options *opt, pl_camera_pose *pose, double *focal, uint8_t *inliers, const pl_device_mask *mask,
                     const MaskDest *ranked_dest, pl_ransac_stats *stats, size_t *n_used) {
    if (n_used)
        *n_used = 0;
    if (!pp || !pose || !focal)
        return fail(PL_ERR_INVALID, "null argument");
    int rc = validate_options(opt);
    if (rc == PL_OK)
        rc = uncal_check_plain(x1, 2, x2, 2, scores, mask, n);
    Context *c = nullptr;
    if (rc == PL_OK)
        rc = get_context(&c);
    if (rc == PL_OK)
        rc = uncal_check_device(c, x1, x2, scores, mask, n);
    if (rc != PL_OK)
        return rc;
    pl_ransac_stats local;
    pl_ransac_stats *st = stats ? stats : &local;
    UncalRows rows;
    rc = rows.stage(c, x1, x2, scores, mask, n);
    if (rc != PL_OK)
        return rc;
    // normalization_about's sum, over the rows the run uses and in their order
    double scale = 0.0;
    if (rows.used) {
        PointStatsRecord rec = {};
        rc = uncal_point_stats(c, rows.used, 2, pp[0], pp[1], &rec);
        scale = rec.scale;
    } else {
        scale = mean_distance_scale(0.0, 0); // (no rows: what the host's empty loop leaves)
    }
    if (rc == PL_OK) {
        PrepareArgs prep;
        prepare_about(pp[0], pp[1], scale, prep);
        MaskDestScope scope(ranked_dest ? ranked_dest : rows.mask_dest());
        rc = shared_focal_run(c, nullptr, nullptr, rows.used, prep, scale, /*resident=*/true, opt, pose, focal,
                              ranked_dest ? nullptr : rows.run_mask(inliers), st);
    }
    rows.finish(c, rc == PL_OK ? inliers : nullptr, rc == PL_OK ? n_used : nullptr);
    return rc;
}

} // namespace

int pl_estimate_shared_focal_relative_pose_dev(const pl_device_points *x1, const pl_device_points *x2, const pl_device_scores *scores,
                                               size_t n, const double *pp, const pl_robust_options *opt, pl_camera_pose *pose, double *focal,
                                               uint8_t *inliers, const pl_device_mask *mask, pl_ransac_stats *stats, size_t *n_used) {
    return shared_focal_dev(x1, x2, scores, n, pp, opt, pose, focal, inliers, mask, nullptr, stats, n_used);
}

int pl_debug_point_stats_about_group_dev(const pl_device_points *x1, const pl_device_points *x2, const size_t *n, const double *centres,
                                         size_t count, double *out) {
    if (!out || !x1 || !x2 || !n || !centres)
        return fail(PL_ERR_INVALID, "a pointer is null");
    if (count == 0)
        return PL_OK;
    if (count > 65535)
        return fail(PL_ERR_INVALID, "too many members");
    int rc = PL_OK;
    for (size_t i = 0; i < count && rc == PL_OK; ++i) {
        rc = check_points_plain(&x1[i], n[i], 2);
        if (rc == PL_OK)
            rc = check_points_plain(&x2[i], n[i], 2);
    }
    Context *c = nullptr;
    if (rc == PL_OK)
        rc = get_context(&c);
    DeviceAllocationCache allocations;
    for (size_t i = 0; i < count && rc == PL_OK; ++i) {
        rc = allocations.check(c, &x1[i], n[i]);
        if (rc == PL_OK)
            rc = allocations.check(c, &x2[i], n[i]);
    }
    if (rc != PL_OK)
        return rc;
    std::vector<AboutStatsMember> m(count);
    for (size_t i = 0; i < count; ++i)
        m[i].a = &x1[i], m[i].b = &x2[i], m[i].n = n[i], m[i].cx = centres[2 * i], m[i].cy = centres[2 * i + 1];
    PointStatsRecord *h_rec = nullptr, *d_rec = nullptr;
    rc = enqueue_about_stats_g(c, c->h_pstats, c->raw_a, m.data(), (uint32_t)count, &h_rec, &d_rec);
    if (rc != PL_OK)
        return rc;
    HIP_TRY(wait_stream(c));
    for (size_t i = 0; i < count; ++i)
        out[2 * i] = n[i] ? h_rec[i].scale : 0.0, out[2 * i + 1] = n[i] ? h_rec[i].absmax : 0.0;
    return PL_OK;
}

int pl_estimate_1D_radial_absolute_pose_dev(const pl_device_points *points2D, const pl_device_points *points3D, const pl_device_scores *scores,
                                            size_t n, const pl_robust_options *opt, pl_camera_pose *pose, uint8_t *inliers,
                                            const pl_device_mask *mask, pl_ransac_stats *stats, size_t *n_used) {
    if (n_used)
        *n_used = 0;
    int rc = validate_options(opt);
    if (rc != PL_OK)
        return rc;
    if (!pose)
        return fail(PL_ERR_INVALID, "points / pose pointer is null");
    rc = uncal_check_plain(points2D, 2, points3D, 3, scores, mask, n);
    if (rc != PL_OK)
        return rc;
    pl_ransac_stats local;
    pl_ransac_stats *st = stats ? stats : &local;
    if (n < 5 && !scores && !mask) { // (the host form: default stats, nothing is read - and here no device is asked for)
        std::memset(st, 0, sizeof(*st));
        return PL_OK;
    }
    Context *c = nullptr;
    rc = get_context(&c);
    if (rc == PL_OK)
        rc = uncal_check_device(c, points2D, points3D, scores, mask, n);
    if (rc != PL_OK)
        return rc;
    UncalRows rows;
    rc = rows.stage(c, points2D, points3D, scores, mask, n);
    if (rc != PL_OK)
        return rc;
    const size_t m = rows.used;
    if (m < 5) { // too few rows (left): default stats, the pose untouched; a device mask keeps the zeros of its fill
        std::memset(st, 0, sizeof(*st));
        const hipError_t e = mask ? wait_stream(c) : hipSuccess;
        rows.finish(c, inliers, n_used);
        return e == hipSuccess ? PL_OK : fail(PL_ERR_HIP, "the fill of the device mask", e);
    }
    // n / sum |x_k| in index order and max |x * scale| of the block (make_problem's bound), then the block itself: the pixels times the
    // scale, the 3-D points as they are
    PointStatsRecord rec = {};
    rc = uncal_point_stats(c, m, 3, 0.0, 0.0, &rec);
    const double scale = rec.scale;
    const int nd = point_doubles(EST_RAD1D);
    hipError_t e = hipSuccess;
    if (rc == PL_OK)
        e = c->pts_arena.ensure(sizeof(double) * nd * m);
    if (rc == PL_OK && e == hipSuccess) {
        const pl_device_points a = ranked_points(c->raw_src_a, 2, m), b = ranked_points(c->raw_src_b, 3, m); // (contiguous fp64, whatever came in)
        e = launch_ingest_soa(ingest_src(&a), ingest_src(&b), (uint32_t)m, 0, c->pts_arena.as<double>(), nullptr, c->stream, scale);
    }
    if (rc == PL_OK && e != hipSuccess)
        rc = fail(PL_ERR_HIP, "the block of scaled pixels", e);
    if (rc != PL_OK) {
        rows.finish(c, nullptr, nullptr);
        return rc;
    }
    pl_problem p;
    p.kind = EST_RAD1D;
    p.device = c->device;
    p.n = (uint32_t)m;
    p.d_pts = c->pts_arena.as<double>();
    p.borrowed = true;
    std::memset(&p.ps, 0, sizeof(p.ps));
    p.ps.n = (uint32_t)m;
    for (int d = 0; d < nd; ++d)
        p.ps.a[d] = p.d_pts + (size_t)d * m;
    p.ps.xy_absmax = std::nextafter((float)rec.absmax, std::numeric_limits<float>::infinity());
    {
        MaskDestScope scope(rows.mask_dest());
        rc = radial1d_run(c, &p, scale, opt, pose, rows.run_mask(inliers), st);
    }
    rows.finish(c, rc == PL_OK ? inliers : nullptr, rc == PL_OK ? n_used : nullptr);
    return rc;
}
