// poselib_amd — the *_dev entry points: correspondences in the caller's DEVICE memory (pl_device_points: fp32 or fp64, strided
// rows).  Included by driver.cc inside extern "C", behind the host front-ends.
//
// Device input goes in front of the existing preparation and produces exactly what the host path would have uploaded:
//   k_ingest        the caller's rows -> contiguous fp64 AoS in Context::raw_a / raw_b (an fp64 set with row_stride == cols is read
//                   where it lies), which is what k_prepare / k_prepare_tangent take: make_problem_prepared(resident = true)
//   k_point_stats   the numbers the host front-ends compute in passes over the caller's arrays - the two order-dependent
//                   reductions of the homography / fundamental normalisation and the pre-filters' bound - one small record back
//   k_ingest_soa    a resident problem's block, written on the device
//   k_ingest_g, k_point_stats_g   the first two for all members of a lock-step group at once (pl_estimate_batch_dev:
//                   group_stage_device below, called by run_group; the entry point itself is in driver_batch.inc)
// From there both kinds of call run the same code (absolute_pose_run, two_view_run), so a _dev call returns the host call's bits.
// Every check of the descriptors happens before the first launch: a caller's mistake is an error code, never a kernel reading a
// host address.

namespace {

// the checks that need no device
int check_points_plain(const pl_device_points *d, size_t n, int cols) {
    if (!d)
        return fail(PL_ERR_INVALID, "device points: descriptor is null");
    if (n > 0x7fffffffu)
        return fail(PL_ERR_INVALID, "too many correspondences");
    if (d->cols != cols)
        return fail(PL_ERR_INVALID, cols == 3 ? "device points: cols must be 3 for this argument" : "device points: cols must be 2 for this argument");
    if (d->dtype != PL_F64 && d->dtype != PL_F32)
        return fail(PL_ERR_INVALID, "device points: dtype must be PL_F64 or PL_F32");
    if (d->row_stride < d->cols)
        return fail(PL_ERR_INVALID, "device points: row_stride (elements) is below cols");
    if (d->row_stride > ((int64_t)1 << 28)) // (n * row_stride * 8 stays far inside 64 bits)
        return fail(PL_ERR_INVALID, "device points: row_stride beyond 2^28 elements");
    if (!d->data && n)
        return fail(PL_ERR_INVALID, "device points: data is null");
    const uintptr_t elt = d->dtype == PL_F32 ? sizeof(float) : sizeof(double);
    if (reinterpret_cast<uintptr_t>(d->data) % elt)
        return fail(PL_ERR_INVALID, "device points: data is not aligned to its element size");
    return PL_OK;
}
// ... and what the runtime knows about the address: device memory of the calling thread's device that holds every row (n > 0)
// the allocation behind an address: device memory of the calling thread's device, and its extent
struct DeviceAllocation {
    uintptr_t lo = 0;
    size_t size = 0;
};
int find_device_allocation(const Context *c, const void *data, DeviceAllocation *out) {
    hipPointerAttribute_t attr;
    std::memset(&attr, 0, sizeof(attr));
    const hipError_t e = hipPointerGetAttributes(&attr, data);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(PL_ERR_INVALID, "device points: data is not an address the HIP runtime knows (a host pointer?)");
    }
    if (attr.isManaged || attr.type == hipMemoryTypeManaged)
        return fail(PL_ERR_INVALID, "device points: data is managed memory, device memory is required");
    if (attr.type != hipMemoryTypeDevice)
        return fail(PL_ERR_INVALID, "device points: data is host memory, device memory is required");
    if (attr.device != c->device)
        return fail(PL_ERR_INVALID, "device points: data lives on another device than the calling thread's (pl_set_device)");
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, const_cast<void *>(data)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(PL_ERR_INVALID, "device points: the allocation behind data cannot be found");
    }
    out->lo = reinterpret_cast<uintptr_t>(base);
    out->size = size;
    return PL_OK;
}
// ... holds every row
int check_points_extent(const DeviceAllocation &al, const pl_device_points *d, size_t n) {
    const size_t elt = d->dtype == PL_F32 ? sizeof(float) : sizeof(double);
    const size_t need = ((n - 1) * (size_t)d->row_stride + (size_t)d->cols) * elt;
    const uintptr_t at = reinterpret_cast<uintptr_t>(d->data);
    if (at < al.lo || at - al.lo > al.size || need > al.size - (at - al.lo))
        return fail(PL_ERR_INVALID, "device points: the rows reach beyond the allocation behind data");
    return PL_OK;
}
// ... the same for `need` bytes at an address (a mask destination: no element type)
int check_bytes_extent(const DeviceAllocation &al, const void *data, size_t need) {
    if (!range_inside(reinterpret_cast<uintptr_t>(data), need, al.lo, al.size))
        return fail(PL_ERR_INVALID, "device points: the rows reach beyond the allocation behind data");
    return PL_OK;
}
int check_points_device(const Context *c, const pl_device_points *d, size_t n) {
    if (n == 0)
        return PL_OK;
    DeviceAllocation al;
    const int rc = find_device_allocation(c, d->data, &al);
    return rc != PL_OK ? rc : check_points_extent(al, d, n);
}
// The same check for the many descriptors of one batch call, which commonly are views into a few allocations: the runtime is asked
// once per allocation, every further address inside a known one only has its extent compared.
struct DeviceAllocationCache {
    std::vector<DeviceAllocation> known;
    size_t last = 0;
    int check(const Context *c, const pl_device_points *d, size_t n) {
        if (n == 0)
            return PL_OK;
        const uintptr_t at = reinterpret_cast<uintptr_t>(d->data);
        for (size_t k = 0; k < known.size(); ++k) {
            const DeviceAllocation &al = known[(last + k) % known.size()];
            if (at >= al.lo && at - al.lo < al.size) {
                last = (last + k) % known.size();
                return check_points_extent(al, d, n);
            }
        }
        DeviceAllocation al;
        const int rc = find_device_allocation(c, d->data, &al);
        if (rc != PL_OK)
            return rc;
        known.push_back(al);
        last = known.size() - 1;
        return check_points_extent(al, d, n);
    }
    // ... for `need` > 0 bytes at an address
    int check_bytes(const Context *c, const void *data, size_t need) {
        const uintptr_t at = reinterpret_cast<uintptr_t>(data);
        for (size_t k = 0; k < known.size(); ++k) {
            const DeviceAllocation &al = known[(last + k) % known.size()];
            if (at >= al.lo && at - al.lo < al.size) {
                last = (last + k) % known.size();
                return check_bytes_extent(al, data, need);
            }
        }
        DeviceAllocation al;
        const int rc = find_device_allocation(c, data, &al);
        if (rc != PL_OK)
            return rc;
        known.push_back(al);
        last = known.size() - 1;
        return check_bytes_extent(al, data, need);
    }
};

// ---- an inlier mask's destination in the caller's device memory (pl_device_mask): the points' checks
int check_mask_plain(const pl_device_mask *d, size_t n) {
    if (!d)
        return fail(PL_ERR_INVALID, "device mask: descriptor is null");
    if (n > 0x7fffffffu)
        return fail(PL_ERR_INVALID, "too many correspondences");
    if (d->stride < 1)
        return fail(PL_ERR_INVALID, "device mask: stride (bytes) is below 1");
    if (d->stride > ((int64_t)1 << 31)) // (n * stride stays far inside 64 bits)
        return fail(PL_ERR_INVALID, "device mask: stride beyond 2^31 bytes");
    if (!d->data && n)
        return fail(PL_ERR_INVALID, "device mask: data is null");
    return PL_OK;
}
int name_the_mask(int rc) {
    if (rc != PL_OK) {
        const size_t at = g_err.find("device points");
        if (at != std::string::npos)
            g_err.replace(at, 13, "device mask");
    }
    return rc;
}
size_t mask_bytes(const pl_device_mask *d, size_t n) { return (n - 1) * (size_t)d->stride + 1; } // (n > 0)
int check_mask_device(const Context *c, const pl_device_mask *d, size_t n) {
    if (n == 0)
        return PL_OK;
    DeviceAllocation al;
    const int rc = find_device_allocation(c, d->data, &al);
    return name_the_mask(rc != PL_OK ? rc : check_bytes_extent(al, d->data, mask_bytes(d, n)));
}
// Zero flags in the destinations of `count` members (data == null or n == 0: none), enqueued on the context's stream: what a
// destination holds for the rows the scores drop and for an item whose host form writes no mask.  The runs that follow on other
// streams need a wait in between; a run on this stream does not.
int enqueue_mask_fill(Context *c, const MaskFillArgs *members, size_t count) {
    uint32_t max_n = 0;
    for (size_t i = 0; i < count; ++i)
        if (members[i].data)
            max_n = std::max(max_n, members[i].n);
    if (!max_n)
        return PL_OK;
    HIP_TRY(c->h_mask_fill.ensure(sizeof(MaskFillArgs) * count));
    std::memcpy(c->h_mask_fill.p, members, sizeof(MaskFillArgs) * count);
    HIP_TRY(launch_mask_fill_g(c->h_mask_fill.dev<MaskFillArgs>(), (uint32_t)count, max_n, c->stream));
    return PL_OK;
}

IngestSrc ingest_src(const pl_device_points *d) {
    IngestSrc s;
    s.data = d->data;
    s.row_stride = d->row_stride;
    s.f32 = d->dtype == PL_F32;
    s.cols = d->cols;
    return s;
}
bool reads_in_place(const pl_device_points *d) { return d->dtype == PL_F64 && d->row_stride == d->cols; }

// plain checks of both sets, the context, the device checks: everything in front of the first launch
int open_device_points(const pl_device_points *a, int cols_a, const pl_device_points *b, int cols_b, size_t n, Context **c) {
    int rc = check_points_plain(a, n, cols_a);
    if (rc == PL_OK)
        rc = check_points_plain(b, n, cols_b);
    if (rc == PL_OK)
        rc = get_context(c);
    if (rc == PL_OK)
        rc = check_points_device(*c, a, n);
    if (rc == PL_OK)
        rc = check_points_device(*c, b, n);
    return rc;
}

// the fp64 AoS blocks of both sets: c->raw_src_a / raw_src_b (k_prepare's input) - the caller's memory where it already is one.
// b == null (the diagnostic of the radial reduction): the first set alone
int ingest_points(Context *c, const pl_device_points *a, const pl_device_points *b, size_t n) {
    c->raw_src_a = c->raw_src_b = nullptr;
    if (n == 0)
        return PL_OK;
    double *out_a = nullptr, *out_b = nullptr;
    if (!reads_in_place(a)) {
        HIP_TRY(c->raw_a.ensure(sizeof(double) * a->cols * n));
        out_a = c->raw_a.as<double>();
    }
    if (b && !reads_in_place(b)) {
        HIP_TRY(c->raw_b.ensure(sizeof(double) * b->cols * n));
        out_b = c->raw_b.as<double>();
    }
    HIP_TRY(launch_ingest(ingest_src(a), ingest_src(b ? b : a), (uint32_t)n, out_a, out_b, c->stream));
    c->raw_src_a = out_a ? out_a : static_cast<const double *>(a->data);
    c->raw_src_b = out_b ? out_b : b ? static_cast<const double *>(b->data) : nullptr;
    return PL_OK;
}

// centre and focal lengths of a camera whose un-projection is (x - c) / f (host_xy_absmax, host_two_view_absmax); false: another model
bool linear_camera_terms(const CameraParams &cam, double &cx, double &cy, double &fx, double &fy) {
    cx = cy = 0, fx = fy = 1;
    if (cam.model_id == CAM_SIMPLE_PINHOLE)
        fx = fy = cam.p[0], cx = cam.p[1], cy = cam.p[2];
    else if (cam.model_id == CAM_PINHOLE)
        fx = cam.p[0], fy = cam.p[1], cx = cam.p[2], cy = cam.p[3];
    else if (cam.model_id != CAM_NULL)
        return false;
    return true;
}

// k_point_stats on the ingested blocks, and its record
void point_stats_sizes(PointStatsArgs &args, size_t n) {
    args.n_as_double = static_cast<double>(n);
    args.scale_divisor = std::sqrt(2) * n;
}
int run_point_stats(Context *c, size_t n, PointStatsArgs args, PointStatsRecord *rec) {
    point_stats_sizes(args, n);
    HIP_TRY(c->h_pstats.ensure(sizeof(PointStatsRecord)));
    HIP_TRY(launch_point_stats(c->raw_src_a, c->raw_src_b, (uint32_t)n, args, c->h_pstats.dev<PointStatsRecord>(), c->stream));
    HIP_TRY(wait_stream(c));
    std::memcpy(rec, c->h_pstats.p, sizeof(*rec));
    return PL_OK;
}
// the raw maximum as the host passes finish it (host_xy_absmax / host_two_view_absmax)
float bound_from_max(double m, bool nan_is_unbounded) {
    const float inf = std::numeric_limits<float>::infinity();
    if (nan_is_unbounded && m != m)
        return inf;
    m = m * (1.0 + 1e-12);
    return std::nextafter((float)m, inf);
}

// What front_begin and host_prefilter_bound take from the host arrays, from the ingested blocks instead: the reductions of the
// normalisation (homography, fundamental) and the pre-filters' bound, in the same cases - absolute pose through a linear camera,
// two-view problems from 1024 correspondences with linear cameras (an absolute-pose problem of a non-linear camera reads k_prepare's
// maximum back: make_problem_prepared, as in the host call).  No launch where the host has no pass either.
// The cases, as k_point_stats' arguments - one function for the single call (device_front_stats) and for the members of a group
// (group_stage_device), whose kernel takes them from a table.  false: the host has no pass over this problem's points.
bool front_stats_plan(int kind, size_t n, const pl_robust_options &opt, const pl_camera *camera1, const pl_camera *camera2,
                      PointStatsArgs &args) {
    std::memset(&args, 0, sizeof(args));
    if (n == 0)
        return false;
    point_stats_sizes(args, n);
    if (kind == EST_ABS) {
        const CameraParams cam = to_cam(camera1);
        if (prefilter_bound_on_device(kind, prepare_unproject(cam, nullptr)))
            return false;
        args.bound = 1;
        linear_camera_terms(cam, args.cx1, args.cy1, args.fx1, args.fy1);
        return true;
    }
    if (kind == EST_REL) {
        if (n < 1024 || !linear_camera_terms(to_cam(camera1), args.cx1, args.cy1, args.fx1, args.fy1) ||
            !linear_camera_terms(to_cam(camera2), args.cx2, args.cy2, args.fx2, args.fy2))
            return false;
        args.bound = 2;
        return true;
    }
    if (kind != EST_FUND && kind != EST_HOM) // (tangent Sampson: its pre-filter takes no bound)
        return false;
    args.norm = 1;
    args.centred = front_centred(kind, opt) ? 1 : 0;
    args.bound = n >= 1024 ? 3 : 0;
    return true;
}
// ... and what the front-end takes from the record of a planned pass
void front_stats_take(const PointStatsArgs &args, const PointStatsRecord &rec, PointNorm *norm, float *bound) {
    if (args.norm)
        norm->c1x = rec.c1x, norm->c1y = rec.c1y, norm->c2x = rec.c2x, norm->c2y = rec.c2y, norm->scale = rec.scale;
    if (args.bound)
        *bound = bound_from_max(rec.absmax, /*nan_is_unbounded=*/args.bound != 1);
}
int device_front_stats(Context *c, int kind, size_t n, const pl_robust_options &opt, const pl_camera *camera1, const pl_camera *camera2,
                       PointNorm *norm, float *bound) {
    *bound = std::numeric_limits<float>::infinity();
    PointStatsArgs args;
    if (!front_stats_plan(kind, n, opt, camera1, camera2, args))
        return PL_OK;
    PointStatsRecord rec;
    const int rc = run_point_stats(c, n, args, &rec);
    if (rc == PL_OK)
        front_stats_take(args, rec, norm, bound);
    return rc;
}

// Stage A of a lock-step group whose members' points are in the caller's device memory (pl_estimate_batch_dev; run_group): ONE
// k_ingest_g launch writes the members that are not contiguous fp64 into their slices of the group's raw block (the others are
// read where they lie), ONE k_point_stats_g launch makes the host's passes of all members, one synchronisation brings every
// record back (the kernel writes them into pinned memory itself); then the front-end arithmetic per member, from its record.
// No pinned staging block and no upload of points.  `resume` (a regrouped long run): the front-ends are complete, only the raw
// blocks are formed again.
int group_stage_device(Context *c, GroupContext &gc, GroupItem *const *pit, uint32_t count, bool resume) {
    HIP_TRY(gc.h_ingest.ensure(sizeof(IngestGroupArgs) * count));
    IngestGroupArgs *hi = gc.h_ingest.as<IngestGroupArgs>();
    uint32_t ingest_n = 0;
    for (uint32_t i = 0; i < count; ++i) {
        GroupItem &g = (*pit[i]);
        const pl_device_points &a = g.ditem->a, &b = g.ditem->b;
        std::memset(&hi[i], 0, sizeof(hi[i]));
        double *out_a = reads_in_place(&a) ? nullptr : gc.raw.as<double>() + g.raw_a_off;
        double *out_b = reads_in_place(&b) ? nullptr : gc.raw.as<double>() + g.raw_b_off;
        g.raw_a = out_a ? out_a : static_cast<const double *>(a.data);
        g.raw_b = out_b ? out_b : static_cast<const double *>(b.data);
        if (!out_a && !out_b)
            continue;
        hi[i].a = ingest_src(&a), hi[i].b = ingest_src(&b);
        hi[i].n = g.n;
        hi[i].out_a = out_a, hi[i].out_b = out_b;
        ingest_n = std::max(ingest_n, g.n);
    }
    HIP_TRY(launch_ingest_g(gc.h_ingest.dev<IngestGroupArgs>(), count, ingest_n, c->stream));
    if (resume)
        return PL_OK;
    HIP_TRY(gc.h_pstats_args.ensure(sizeof(PointStatsGroupArgs) * count));
    HIP_TRY(gc.h_pstats.ensure(sizeof(PointStatsRecord) * count));
    PointStatsGroupArgs *hs = gc.h_pstats_args.as<PointStatsGroupArgs>();
    bool any = false;
    for (uint32_t i = 0; i < count; ++i) {
        GroupItem &g = (*pit[i]);
        const pl_batch_item &it = *g.item;
        std::memset(&hs[i], 0, sizeof(hs[i]));
        if (!front_stats_plan(g.kind, g.n, *it.opt, it.camera1, it.camera2, hs[i].args))
            continue;
        hs[i].a_raw = g.raw_a, hs[i].b_raw = g.raw_b;
        hs[i].n = g.n;
        hs[i].out = gc.h_pstats.dev<PointStatsRecord>() + i;
        any = true;
    }
    if (any) {
        HIP_TRY(launch_point_stats_g(gc.h_pstats_args.dev<PointStatsGroupArgs>(), count, c->stream));
        HIP_TRY(wait_stream(c));
    }
    const PointStatsRecord *rec = gc.h_pstats.as<PointStatsRecord>();
    for (uint32_t i = 0; i < count; ++i) {
        GroupItem &g = (*pit[i]);
        const pl_batch_item &it = *g.item;
        PointNorm norm;
        float bound = std::numeric_limits<float>::infinity();
        if (hs[i].n)
            front_stats_take(hs[i].args, rec[i], &norm, &bound);
        front_begin_with(g.fe, g.kind, norm, *it.opt, it.camera1, it.camera2);
        g.xy_absmax = bound;
        g.have_absmax = true;
        g.prepared = true;
    }
    return PL_OK;
}

// What a *_dev entry point says about its options and cameras before it looks at the points (kinds 0 - 3); the scored forms
// (driver_scored.inc) say the same, first.
int dev_entry_precheck(int kind, const pl_robust_options *opt, const pl_camera *camera1, const pl_camera *camera2) {
    static const char *const unsupported_camera = "camera model not supported (NULL, SIMPLE_PINHOLE, PINHOLE, SIMPLE_RADIAL, RADIAL, OPENCV, OPENCV_FISHEYE, SIMPLE_RADIAL_FISHEYE, RADIAL_FISHEYE)";
    if (kind == EST_ABS) {
        const int rc = validate_options(opt, /*focal_entry=*/true);
        if (rc != PL_OK)
            return rc;
        if (opt->estimate_focal_length) // (its loop and compute_max_focal_length read the image points on the host)
            return fail(PL_ERR_UNSUPPORTED, "estimate_focal_length is not served from device memory: use pl_estimate_absolute_pose");
        if (!camera1 || !camera_supported(camera1))
            return fail(PL_ERR_UNSUPPORTED, unsupported_camera);
        return PL_OK;
    }
    if (kind != EST_REL)
        return validate_options(opt);
    const bool tangent = opt && opt->tangent_sampson; // (as pl_estimate_relative_pose)
    pl_robust_options plain;
    if (tangent) {
        plain = *opt;
        plain.tangent_sampson = 0;
    }
    const int rc = validate_options(tangent ? &plain : opt);
    if (rc != PL_OK)
        return rc;
    if (tangent && (opt->bundle.refine_focal_length || opt->bundle.refine_principal_point || opt->bundle.refine_extra_params))
        return fail(PL_ERR_UNSUPPORTED, "tangent_sampson with bundle.refine_focal_length / refine_principal_point / refine_extra_params "
                                        "refines the intrinsics with the pose (CameraRelativePoseRefiner): not served, fixed cameras only");
    if (!camera1 || !camera2 || !camera_supported(camera1) || !camera_supported(camera2))
        return fail(PL_ERR_UNSUPPORTED, unsupported_camera);
    return PL_OK;
}

int estimate_two_view_dev(int kind, const pl_device_points *x1, const pl_device_points *x2, size_t n, const pl_camera *camera1,
                          const pl_camera *camera2, const pl_robust_options *opt, void *model, uint8_t *inliers, pl_ransac_stats *st) {
    Context *c;
    int rc = open_device_points(x1, 2, x2, 2, n, &c);
    if (rc == PL_OK)
        rc = ingest_points(c, x1, x2, n);
    PointNorm norm;
    float bound;
    if (rc == PL_OK)
        rc = device_front_stats(c, kind, n, *opt, camera1, camera2, &norm, &bound);
    if (rc != PL_OK)
        return rc;
    FrontEnd fe;
    front_begin_with(fe, kind, norm, *opt, camera1, camera2);
    rc = two_view_run(c, fe, kind, nullptr, nullptr, n, &bound, model, inliers, st);
    c->raw_src_a = c->raw_src_b = nullptr; // (the caller's memory is not read after the call)
    return rc;
}

} // namespace

int pl_debug_check_device_points(const pl_device_points *d, size_t n, int cols) {
    int rc = check_points_plain(d, n, cols);
    if (rc != PL_OK || n == 0)
        return rc;
    Context *c;
    rc = get_context(&c);
    if (rc != PL_OK)
        return rc;
    return check_points_device(c, d, n);
}

int pl_debug_point_stats_dev(const pl_device_points *x1, const pl_device_points *x2, size_t n, int centroid, double *out) {
    if (!out)
        return fail(PL_ERR_INVALID, "output pointer is null");
    Context *c;
    int rc = open_device_points(x1, 2, x2, 2, n, &c);
    if (rc != PL_OK)
        return rc;
    for (int i = 0; i < 8; ++i)
        out[i] = 0.0;
    if (n == 0)
        return PL_OK;
    rc = ingest_points(c, x1, x2, n);
    if (rc != PL_OK)
        return rc;
    PointStatsArgs args;
    std::memset(&args, 0, sizeof(args));
    args.norm = 1, args.centred = centroid ? 1 : 0, args.bound = 3;
    PointStatsRecord rec;
    rc = run_point_stats(c, n, args, &rec);
    if (rc != PL_OK)
        return rc;
    out[0] = rec.c1x, out[1] = rec.c1y, out[2] = rec.c2x, out[3] = rec.c2y, out[4] = rec.scale, out[5] = rec.absmax;
    std::memset(&args, 0, sizeof(args));
    args.bound = 1; // the identity camera: |x - 0| / 1
    args.fx1 = args.fy1 = 1.0;
    rc = run_point_stats(c, n, args, &rec);
    if (rc != PL_OK)
        return rc;
    out[6] = rec.absmax;
    return PL_OK;
}

int pl_debug_point_stats_group_dev(const pl_device_points *x1, const pl_device_points *x2, const size_t *n, size_t count, int centroid,
                                   double *out) {
    if (!out || !x1 || !x2 || !n)
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
    const uint32_t G = (uint32_t)count;
    // the members' slices of one raw block (sets that are contiguous fp64 are read where they lie), the two tables, the records
    size_t raw_doubles = 0;
    for (size_t i = 0; i < count; ++i)
        raw_doubles += (reads_in_place(&x1[i]) ? 0 : 2 * n[i]) + (reads_in_place(&x2[i]) ? 0 : 2 * n[i]);
    HIP_TRY(c->raw_a.ensure(sizeof(double) * std::max<size_t>(raw_doubles, 1)));
    const size_t table_bytes = (sizeof(IngestGroupArgs) + sizeof(PointStatsGroupArgs) + sizeof(PointStatsRecord)) * count;
    HIP_TRY(c->h_pstats.ensure(table_bytes));
    PointStatsRecord *rec = c->h_pstats.as<PointStatsRecord>();
    PointStatsGroupArgs *hs = reinterpret_cast<PointStatsGroupArgs *>(rec + count);
    IngestGroupArgs *hi = reinterpret_cast<IngestGroupArgs *>(hs + count);
    PointStatsRecord *d_rec = c->h_pstats.dev<PointStatsRecord>();
    PointStatsGroupArgs *d_hs = reinterpret_cast<PointStatsGroupArgs *>(d_rec + count);
    IngestGroupArgs *d_hi = reinterpret_cast<IngestGroupArgs *>(d_hs + count);
    std::memset(rec, 0, table_bytes);
    size_t at = 0;
    uint32_t ingest_n = 0;
    for (size_t i = 0; i < count; ++i) {
        out[8 * i + 0] = out[8 * i + 1] = out[8 * i + 2] = out[8 * i + 3] = out[8 * i + 4] = out[8 * i + 5] = out[8 * i + 6] = out[8 * i + 7] = 0.0;
        if (n[i] == 0)
            continue;
        double *oa = nullptr, *ob = nullptr;
        if (!reads_in_place(&x1[i]))
            oa = c->raw_a.as<double>() + at, at += 2 * n[i];
        if (!reads_in_place(&x2[i]))
            ob = c->raw_a.as<double>() + at, at += 2 * n[i];
        if (oa || ob) {
            hi[i].a = ingest_src(&x1[i]), hi[i].b = ingest_src(&x2[i]);
            hi[i].n = (uint32_t)n[i];
            hi[i].out_a = oa, hi[i].out_b = ob;
            ingest_n = std::max(ingest_n, (uint32_t)n[i]);
        }
        hs[i].a_raw = oa ? oa : static_cast<const double *>(x1[i].data);
        hs[i].b_raw = ob ? ob : static_cast<const double *>(x2[i].data);
        hs[i].n = (uint32_t)n[i];
        hs[i].out = d_rec + i;
        hs[i].args.norm = 1, hs[i].args.centred = centroid ? 1 : 0, hs[i].args.bound = 3;
        point_stats_sizes(hs[i].args, n[i]);
    }
    HIP_TRY(launch_ingest_g(d_hi, G, ingest_n, c->stream));
    HIP_TRY(launch_point_stats_g(d_hs, G, c->stream));
    HIP_TRY(wait_stream(c));
    for (size_t i = 0; i < count; ++i) {
        if (n[i] == 0)
            continue;
        double *o = out + 8 * i;
        o[0] = rec[i].c1x, o[1] = rec[i].c1y, o[2] = rec[i].c2x, o[3] = rec[i].c2y, o[4] = rec[i].scale, o[5] = rec[i].absmax;
        std::memset(&hs[i].args, 0, sizeof(hs[i].args));
        hs[i].args.bound = 1; // the identity camera: |x - 0| / 1
        hs[i].args.fx1 = hs[i].args.fy1 = 1.0;
        point_stats_sizes(hs[i].args, n[i]);
    }
    HIP_TRY(launch_point_stats_g(d_hs, G, c->stream));
    HIP_TRY(wait_stream(c));
    for (size_t i = 0; i < count; ++i)
        if (n[i])
            out[8 * i + 6] = rec[i].absmax;
    return PL_OK;
}

int pl_estimate_absolute_pose_dev(const pl_device_points *points2D, const pl_device_points *points3D, size_t n,
                                  const pl_robust_options *opt, pl_camera *camera, pl_camera_pose *pose, uint8_t *inliers,
                                  pl_ransac_stats *stats) {
    int rc = dev_entry_precheck(EST_ABS, opt, camera, nullptr);
    if (rc != PL_OK)
        return rc;
    Context *c;
    rc = open_device_points(points2D, 2, points3D, 3, n, &c);
    if (rc == PL_OK)
        rc = ingest_points(c, points2D, points3D, n);
    PointNorm norm;
    float bound;
    if (rc == PL_OK)
        rc = device_front_stats(c, EST_ABS, n, *opt, camera, nullptr, &norm, &bound);
    if (rc != PL_OK)
        return rc;
    FrontEnd fe;
    front_begin_with(fe, EST_ABS, norm, *opt, camera, nullptr);
    rc = absolute_pose_run(c, fe, nullptr, nullptr, n, &bound, opt, camera, pose, inliers, stats);
    c->raw_src_a = c->raw_src_b = nullptr; // (the caller's memory is not read after the call)
    return rc;
}

int pl_estimate_relative_pose_dev(const pl_device_points *x1, const pl_device_points *x2, size_t n, const pl_camera *camera1,
                                  const pl_camera *camera2, const pl_robust_options *opt, pl_camera_pose *pose, uint8_t *inliers,
                                  pl_ransac_stats *stats) {
    const bool tangent = opt && opt->tangent_sampson; // (as pl_estimate_relative_pose)
    const int rc = dev_entry_precheck(EST_REL, opt, camera1, camera2);
    if (rc != PL_OK)
        return rc;
    pl_ransac_stats local;
    return estimate_two_view_dev(tangent ? EST_RELT : EST_REL, x1, x2, n, camera1, camera2, opt, pose, inliers, stats ? stats : &local);
}

int pl_estimate_fundamental_dev(const pl_device_points *x1, const pl_device_points *x2, size_t n, const pl_robust_options *opt, double *F,
                                uint8_t *inliers, pl_ransac_stats *stats) {
    int rc = validate_options(opt);
    if (rc == PL_OK)
        rc = check_points_plain(x1, n, 2);
    if (rc == PL_OK)
        rc = check_points_plain(x2, n, 2);
    if (rc != PL_OK)
        return rc;
    pl_ransac_stats local;
    pl_ransac_stats *st = stats ? stats : &local;
    if (n < 7) { // robust.cc:548-550: nothing is read
        std::memset(st, 0, sizeof(*st));
        st->model_score = std::numeric_limits<double>::max();
        return PL_OK;
    }
    return estimate_two_view_dev(EST_FUND, x1, x2, n, nullptr, nullptr, opt, F, inliers, st);
}

int pl_estimate_homography_dev(const pl_device_points *x1, const pl_device_points *x2, size_t n, const pl_robust_options *opt, double *H,
                               uint8_t *inliers, pl_ransac_stats *stats) {
    int rc = validate_options(opt);
    if (rc == PL_OK)
        rc = check_points_plain(x1, n, 2);
    if (rc == PL_OK)
        rc = check_points_plain(x2, n, 2);
    if (rc != PL_OK)
        return rc;
    pl_ransac_stats local;
    pl_ransac_stats *st = stats ? stats : &local;
    if (n < 4) { // robust.cc:716-718
        std::memset(st, 0, sizeof(*st));
        st->model_score = std::numeric_limits<double>::max();
        return PL_OK;
    }
    return estimate_two_view_dev(EST_HOM, x1, x2, n, nullptr, nullptr, opt, H, inliers, st);
}

// pl_problem_create from device memory: k_ingest_soa writes the block and takes make_problem's maximum
int pl_problem_create_dev(int kind, const pl_device_points *a, const pl_device_points *b, size_t n, pl_problem **out) {
    if (!out)
        return fail(PL_ERR_INVALID, "output pointer is null");
    if ((kind < 0 || kind > 3) && kind != EST_RAD1D)
        return fail(PL_ERR_INVALID, "unknown problem kind");
    const bool two_view = kind != EST_ABS && kind != EST_RAD1D;
    Context *c;
    int rc = open_device_points(a, 2, b, two_view ? 2 : 3, n, &c);
    if (rc != PL_OK)
        return rc;
    pl_problem *p = new pl_problem();
    p->kind = kind;
    p->device = c->device;
    p->n = (uint32_t)n;
    p->d_pts = nullptr;
    std::memset(&p->ps, 0, sizeof(p->ps));
    p->ps.n = (uint32_t)n;
    *out = p;
    if (n == 0)
        return PL_OK;
    const int nd = point_doubles(kind);
    hipError_t e = c->absmax.ensure(sizeof(unsigned long long));
    if (e == hipSuccess)
        e = c->h_absmax.ensure(sizeof(unsigned long long));
    if (e == hipSuccess)
        e = hipMalloc((void **)&p->d_pts, sizeof(double) * nd * n);
    if (e == hipSuccess)
        e = hipMemsetAsync(c->absmax.p, 0, sizeof(unsigned long long), c->stream);
    if (e == hipSuccess)
        e = launch_ingest_soa(ingest_src(a), ingest_src(b), (uint32_t)n, two_view ? 1 : 0, p->d_pts, c->absmax.as<unsigned long long>(),
                              c->stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(c->h_absmax.p, c->absmax.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess)
        e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        if (p->d_pts)
            (void)hipFree(p->d_pts);
        delete p;
        *out = nullptr;
        return fail(PL_ERR_HIP, "ingestion of the correspondences", e);
    }
    for (int d = 0; d < nd; ++d)
        p->ps.a[d] = p->d_pts + (size_t)d * n;
    double amax;
    std::memcpy(&amax, c->h_absmax.p, sizeof(double));
    p->ps.xy_absmax = std::nextafter((float)amax, std::numeric_limits<float>::infinity());
    return PL_OK;
}

int pl_problem_create_tangent_dev(const pl_device_points *x1, const pl_device_points *x2, size_t n, const pl_camera *camera1,
                                  const pl_camera *camera2, pl_problem **out) {
    if (!out)
        return fail(PL_ERR_INVALID, "output pointer is null");
    if ((camera1 && !camera_supported(camera1)) || (camera2 && !camera_supported(camera2)))
        return fail(PL_ERR_UNSUPPORTED, "camera model outside the supported set (or too few parameters)");
    if (n > 0x7fffffffu / 18)
        return fail(PL_ERR_INVALID, "too many correspondences");
    Context *c;
    int rc = open_device_points(x1, 2, x2, 2, n, &c);
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
    rc = ingest_points(c, x1, x2, n);
    hipError_t e = hipSuccess;
    if (rc == PL_OK) {
        e = hipMalloc((void **)&p->d_pts, sizeof(double) * 18 * n);
        if (e == hipSuccess)
            e = launch_prepare(c->raw_src_a, c->raw_src_b, (uint32_t)n, pa, p->d_pts, nullptr, c->stream);
        if (e == hipSuccess)
            e = hipStreamSynchronize(c->stream);
    }
    c->raw_src_a = c->raw_src_b = nullptr; // (the caller's memory is not read after the call)
    if (rc != PL_OK || e != hipSuccess) {
        if (p->d_pts)
            (void)hipFree(p->d_pts);
        delete p;
        *out = nullptr;
        return rc != PL_OK ? rc : fail(PL_ERR_HIP, "preparation of the tangent-Sampson problem", e);
    }
    p->ps.a[0] = p->d_pts;
    return PL_OK;
}

// ---------------------------------------------------------------------------- un-distortion stage, device memory to device memory
// pl_undistort_points for rows that are in the caller's device memory and stay there: k_undistort_dev / k_undistort_dev_g
// (ingest.hip) read the source through the ingest loader and write the caller's fp64 rows.  The range arithmetic is pl_ranges.h.
namespace {

static const char *const undistort_unsupported_camera = "camera model not supported (SIMPLE_PINHOLE, PINHOLE, SIMPLE_RADIAL, RADIAL, OPENCV, OPENCV_FISHEYE, SIMPLE_RADIAL_FISHEYE, RADIAL_FISHEYE)";
// every supported model but NULL (pl_undistort_points' rule)
int undistort_camera_check(const pl_camera *camera) {
    if (!camera || !camera_supported(camera) || camera->model_id == CAM_NULL)
        return fail(PL_ERR_UNSUPPORTED, undistort_unsupported_camera);
    return PL_OK;
}
// the camera and the distortion-free camera its output pixels belong to
void undistort_camera_terms(const pl_camera *camera, CameraParams &cam, double &fx, double &fy, double &cx, double &cy) {
    cam = to_cam(camera);
    if (!camera_has_two_focals(camera->model_id))
        fx = fy = cam.p[0], cx = cam.p[1], cy = cam.p[2];
    else
        fx = cam.p[0], fy = cam.p[1], cx = cam.p[2], cy = cam.p[3];
}

// the destination as a point set: its memory gets the points' checks, the messages name the destination
pl_device_points out_as_points(const pl_device_points_out *d) {
    pl_device_points p;
    p.data = d->data, p.row_stride = d->row_stride, p.dtype = d->dtype, p.cols = d->cols;
    return p;
}
int name_the_destination(int rc) {
    if (rc != PL_OK) {
        const size_t at = g_err.find("device points");
        if (at != std::string::npos)
            g_err.replace(at, 13, "destination");
    }
    return rc;
}
// the destination's checks that need no device
int check_out_plain(const pl_device_points_out *d, size_t n) {
    if (!d)
        return fail(PL_ERR_INVALID, "destination: descriptor is null");
    if (d->dtype != PL_F64)
        return fail(PL_ERR_INVALID, "destination: dtype must be PL_F64 (fp32 output is not offered)");
    const pl_device_points p = out_as_points(d);
    return name_the_destination(check_points_plain(&p, n, 2)); // (row_stride >= cols == 2, 8-byte alignment, null data, n)
}
// Source and destination together: in place when the destination IS the source (same address, same stride, fp64), otherwise the
// two byte ranges must not share a byte.
int check_undistort_ranges(const pl_device_points *src, const pl_device_points_out *out, size_t n) {
    if (n == 0)
        return PL_OK;
    if (out->data == src->data && out->row_stride == src->row_stride && src->dtype == PL_F64)
        return PL_OK;
    uint64_t src_bytes = 0, out_bytes = 0;
    if (!rows_span_bytes(n, src->row_stride, 2, src->dtype == PL_F32 ? sizeof(float) : sizeof(double), &src_bytes) ||
        !rows_span_bytes(n, out->row_stride, 2, sizeof(double), &out_bytes))
        return fail(PL_ERR_INVALID, "destination: the rows' extent does not fit 64 bits");
    if (ranges_overlap(reinterpret_cast<uintptr_t>(src->data), src_bytes, reinterpret_cast<uintptr_t>(out->data), out_bytes))
        return fail(PL_ERR_INVALID, "destination: overlaps the source (in place needs the same address, the same row_stride and an fp64 source)");
    return PL_OK;
}
int check_undistort_plain(const pl_camera *camera, const pl_device_points *src, size_t n, const pl_device_points_out *out) {
    int rc = undistort_camera_check(camera);
    if (rc == PL_OK)
        rc = check_points_plain(src, n, 2);
    if (rc == PL_OK)
        rc = check_out_plain(out, n);
    if (rc == PL_OK)
        rc = check_undistort_ranges(src, out, n);
    return rc;
}
UndistortDevArgs undistort_dev_args(const pl_camera *camera, const pl_device_points *src, size_t n, const pl_device_points_out *out) {
    UndistortDevArgs a;
    std::memset(&a, 0, sizeof(a));
    a.src = ingest_src(src);
    a.n = (uint32_t)n;
    undistort_camera_terms(camera, a.cam, a.fx, a.fy, a.cx, a.cy);
    a.out = static_cast<double *>(out->data);
    a.out_stride = out->row_stride;
    return a;
}

} // namespace

int pl_undistort_points_dev(const pl_camera *camera, const pl_device_points *points2D, size_t n, const pl_device_points_out *out) {
    int rc = check_undistort_plain(camera, points2D, n, out);
    Context *c = nullptr;
    if (rc == PL_OK)
        rc = get_context(&c);
    if (rc != PL_OK || n == 0)
        return rc;
    rc = check_points_device(c, points2D, n);
    if (rc == PL_OK) {
        const pl_device_points p = out_as_points(out);
        rc = name_the_destination(check_points_device(c, &p, n));
    }
    if (rc != PL_OK)
        return rc;
    HIP_TRY(launch_undistort_dev(undistort_dev_args(camera, points2D, n, out), c->stream));
    HIP_TRY(wait_stream(c));
    return PL_OK;
}

int pl_undistort_points_batch_dev(pl_undistort_item_dev *items, size_t count) {
    if (count == 0)
        return PL_OK;
    if (!items)
        return fail(PL_ERR_INVALID, "items pointer is null");
    if (count > 0x7fffffffu)
        return fail(PL_ERR_INVALID, "too many items");
    std::vector<std::string> cause(count);
    auto decide = [&](size_t i, int rc) { // (rc came from fail(): g_err holds the cause)
        items[i].status = rc;
        cause[i] = g_err;
    };
    auto first_decided = [&]() -> int {
        for (size_t i = 0; i < count; ++i)
            if (items[i].status != PL_OK)
                return fail(items[i].status, ("pl_undistort_points_batch_dev: item " + std::to_string(i) + ": " + cause[i]).c_str());
        return PL_OK;
    };
    for (size_t i = 0; i < count; ++i) {
        items[i].status = PL_OK;
        const int rc = check_undistort_plain(items[i].camera, &items[i].points2D, items[i].n, &items[i].out);
        if (rc != PL_OK)
            decide(i, rc);
    }
    Context *c;
    int rc = get_context(&c);
    if (rc != PL_OK) { // no device: what was decided without one comes first
        const std::string why = g_err;
        const int first = first_decided();
        for (size_t i = 0; i < count; ++i)
            if (items[i].status == PL_OK)
                items[i].status = rc;
        return first != PL_OK ? first : fail(rc, why.c_str());
    }
    DeviceAllocationCache allocations;
    uint32_t max_n = 0;
    for (size_t i = 0; i < count; ++i) {
        if (items[i].status != PL_OK)
            continue;
        rc = allocations.check(c, &items[i].points2D, items[i].n);
        if (rc == PL_OK) {
            const pl_device_points p = out_as_points(&items[i].out);
            rc = name_the_destination(allocations.check(c, &p, items[i].n));
        }
        if (rc != PL_OK)
            decide(i, rc);
        else
            max_n = std::max(max_n, (uint32_t)items[i].n);
    }
    // one table (pinned and mapped: the kernel reads it where it lies), one launch, one synchronisation; a refused or empty item is a
    // member with n == 0
    if (max_n) {
        HIP_TRY(c->h_undistort.ensure(sizeof(UndistortDevArgs) * count));
        UndistortDevArgs *tab = c->h_undistort.as<UndistortDevArgs>();
        for (size_t i = 0; i < count; ++i) {
            if (items[i].status == PL_OK && items[i].n)
                tab[i] = undistort_dev_args(items[i].camera, &items[i].points2D, items[i].n, &items[i].out);
            else
                std::memset(&tab[i], 0, sizeof(tab[i]));
        }
        hipError_t e = launch_undistort_dev_g(c->h_undistort.dev<UndistortDevArgs>(), (uint32_t)count, max_n, c->stream);
        if (e == hipSuccess)
            e = wait_stream(c);
        if (e != hipSuccess) {
            for (size_t i = 0; i < count; ++i)
                if (items[i].status == PL_OK)
                    items[i].status = PL_ERR_HIP;
            return fail(PL_ERR_HIP, "pl_undistort_points_batch_dev: the un-distortion launch", e);
        }
    }
    return first_decided();
}
