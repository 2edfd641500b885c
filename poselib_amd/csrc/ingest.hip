// poselib_amd — correspondences that are already in device memory (pl_device_points, the *_dev entry points) on their way into
// the blocks the existing preparation takes (gfx950).  Everything here sits IN FRONT of k_prepare / a resident problem's SoA
// block and produces exactly what the host path would have uploaded or read back, so nothing behind it changes:
//
//   k_ingest        strided fp32 / fp64 rows -> contiguous fp64 AoS (Context::raw_a / raw_b); fp32 widens exactly
//   k_ingest_soa    the same sources -> the SoA block of a resident problem, with make_problem's max |coordinate|
//   k_point_stats   what the front-ends compute over the raw points on the host: the two ORDER-DEPENDENT reductions of the
//                   homography / fundamental normalisation (utils.cc:584-644: centroid sums, then the mean distance), added
//                   strictly in index order by one wavefront, and the order-free maxima behind the pre-filters' bound; the same
//                   adder for the two front-ends of unknown cameras: the mean distance from a GIVEN centre (shared focal,
//                   normalization_about) and n / sum |x_k| of one point set (1D radial, with max |x * scale| of its block)
//   k_ingest_ranked, k_ingest_ranked_g   k_ingest through a permutation: the rows an item's scores keep, in descending score (rank.hip)
//   k_ingest_g, k_point_stats_g   the two for a lock-step group of problems (pl_estimate_batch_dev): the member is a grid
//                   dimension, its arguments come from a device-visible table; the bodies are those of the single forms
//   k_undistort_dev, k_undistort_dev_g   the un-distortion stage (k_undistort, pipeline.hip) from the caller's rows into the
//                   caller's fp64 rows (pl_undistort_points_dev / _batch_dev): nothing passes through the host
//   k_mask_fill_g   zero flags in the callers' inlier-mask destinations (pl_estimate_dev_masked / _batch_dev_masked), in front of
//                   the runs whose mask launches write the inliers' flags there
//
// The build has -ffp-contract=off, fp64 sqrt and division on the device are IEEE (tests/test_gpu_device_math*): the sums carry
// the host's bits.  The caller's pointers arrive as kernel arguments and are read as global memory (pl_global.h).
#include "pl_kernels.h"
#include "pl_global.h"

namespace pl {

namespace {

// element (row, col) of a source, widened
__device__ __forceinline__ double ingest_load(const void *data, int f32, size_t at) {
    if (f32)
        return (double)as_global(static_cast<const float *>(data))[at];
    return as_global(static_cast<const double *>(data))[at];
}

// non-negative doubles (and NaN, whose pattern is above +inf) order like their bit patterns (prepare_body's idiom)
__device__ __forceinline__ unsigned long long wave_max_bits(double m) {
    unsigned long long bits = (unsigned long long)__double_as_longlong(m);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(bits, off, 64);
        bits = o > bits ? o : bits;
    }
    return bits;
}
__device__ __forceinline__ void take_abs(double &m, double x) {
    const double v = fabs(x);
    m = (v > m || v != v) ? v : m; // NaN propagates, like the host loops
}

} // namespace

// One thread per correspondence: its row of each set, element by element (plain loads; rows are 8 - 24 bytes).  Row i of the
// sources becomes row j of the blocks (j == i but for a ranked item).
__device__ __forceinline__ void ingest_row(const IngestSrc &a, const IngestSrc &b, uint32_t i, uint32_t j, double *__restrict__ out_a,
                                           double *__restrict__ out_b) {
    if (out_a) {
        const size_t row = (size_t)i * (size_t)a.row_stride;
        for (int d = 0; d < a.cols; ++d)
            out_a[(size_t)j * a.cols + d] = ingest_load(a.data, a.f32, row + d);
    }
    if (out_b) {
        const size_t row = (size_t)i * (size_t)b.row_stride;
        for (int d = 0; d < b.cols; ++d)
            out_b[(size_t)j * b.cols + d] = ingest_load(b.data, b.f32, row + d);
    }
}
__global__ __launch_bounds__(256) void k_ingest(IngestSrc a, IngestSrc b, uint32_t n, double *__restrict__ out_a,
                                                double *__restrict__ out_b) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n)
        return;
    ingest_row(a, b, i, i, out_a, out_b);
}
// ... of every member of a group: blockIdx.z is the member, the grid's extent the largest member's.  A member whose sets are both
// read where they lie (out_a == out_b == null) has n == 0 in the table; blocks beyond a member's rows return.
__global__ __launch_bounds__(256) void k_ingest_g(const IngestGroupArgs *tab) {
    const IngestGroupArgs &in = tab[blockIdx.z];
    const uint32_t n = in.n;
    if (blockIdx.x * 256u >= n)
        return;
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n)
        return;
    ingest_row(in.a, in.b, i, i, as_global(in.out_a), as_global(in.out_b)); // (the sources are read as global memory by ingest_load)
}
// ... of an item with scores (rank.hip): output row j is the caller's row order[j], j below the kept count.  Both come from device
// memory - the launch follows the ranking on the stream, no host round trip between them; in.n bounds the grid.
__device__ __forceinline__ void ingest_ranked_body(const IngestRankedArgs &in) {
    if (blockIdx.x * 256u >= in.n)
        return;
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= *as_global(in.kept))
        return;
    ingest_row(in.a, in.b, as_global(in.order)[j], j, as_global(in.out_a), as_global(in.out_b));
}
__global__ __launch_bounds__(256) void k_ingest_ranked(IngestRankedArgs in) { ingest_ranked_body(in); }
__global__ __launch_bounds__(256) void k_ingest_ranked_g(const IngestRankedArgs *tab) { ingest_ranked_body(tab[blockIdx.z]); }

// ... straight into a resident problem's SoA block: a's columns, then b's, n doubles each (make_problem's layout and bound).
// scale_a: factor of a's columns on their way in (the 1D-radial front-end; x * 1.0 == x for everybody else), the bound is taken
// of the product, like make_problem's.  absmax_bits == null: the caller has the bound from elsewhere (k_point_stats, norm 3).
__global__ __launch_bounds__(256) void k_ingest_soa(IngestSrc a, IngestSrc b, uint32_t n, int b_in_max, double scale_a,
                                                    double *__restrict__ soa, unsigned long long *absmax_bits) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    double m = 0.0;
    if (i < n) {
        const size_t ra = (size_t)i * (size_t)a.row_stride, rb = (size_t)i * (size_t)b.row_stride;
        for (int d = 0; d < a.cols; ++d) {
            const double v = ingest_load(a.data, a.f32, ra + d) * scale_a;
            soa[(size_t)d * n + i] = v;
            take_abs(m, v);
        }
        for (int d = 0; d < b.cols; ++d) {
            const double v = ingest_load(b.data, b.f32, rb + d);
            soa[(size_t)(a.cols + d) * n + i] = v;
            if (b_in_max)
                take_abs(m, v);
        }
    }
    const unsigned long long bits = wave_max_bits(m);
    if (absmax_bits && (threadIdx.x & 63) == 0 && bits)
        atomicMax(absmax_bits, bits);
}

// One workgroup per problem.  The sums: all four wavefronts load a chunk of 256 correspondences and form the per-point terms side by
// side (the subtraction and the square root are element-wise) into LDS; wavefront 0 then adds the chunk's terms strictly in index
// order - every lane reads the same word (an LDS broadcast) and carries the same accumulator, so the loads run ahead of the
// dependent additions and the result needs no broadcast.  All four wavefronts then take the maxima, which do not depend on the
// order.
constexpr int kStatsChunk = 256;
// (the body of k_point_stats and of k_point_stats_g: one piece of code, so the sums of the two forms cannot drift apart)
__device__ __forceinline__ void point_stats_body(const double *__restrict__ a_raw, const double *__restrict__ b_raw, uint32_t n,
                                                 const PointStatsArgs &g, PointStatsRecord *__restrict__ out) {
    __shared__ double s_terms[4 * kStatsChunk];
    __shared__ double s_norm[5];
    __shared__ unsigned long long s_max;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool adder = wave == 0;
    if (threadIdx.x == 0)
        s_max = 0ull;
    if (threadIdx.x < 5)
        s_norm[threadIdx.x] = 0.0;
    __syncthreads();
    if (g.norm == 3) { // radial (one point set): sum += sqrt(0.0 + x * x + y * y) in index order, the record carries n / sum
        double sum = 0.0;
        for (uint32_t base = 0; base < n; base += kStatsChunk) {
            const uint32_t i = base + threadIdx.x;
            if (i < n) {
                const double x = a_raw[2 * (size_t)i], y = a_raw[2 * (size_t)i + 1];
                s_terms[threadIdx.x] = sqrt(0.0 + x * x + y * y);
            }
            __syncthreads();
            if (adder) {
                const int count = (int)(n - base < (uint32_t)kStatsChunk ? n - base : (uint32_t)kStatsChunk);
#pragma unroll 8
                for (int k = 0; k < count; ++k)
                    sum += s_terms[k];
            }
            __syncthreads();
        }
        if (threadIdx.x == 0)
            s_norm[4] = g.n_as_double / sum;
    } else if (g.norm) { // (n, and with it every loop bound and barrier below, is the same for the whole workgroup)
        const bool about = g.norm == 2; // about a given centre (shared focal): c1 = (cx1, cy1), c2 = (cx2, cy2) of the arguments
        if (about) {
            if (threadIdx.x == 0)
                s_norm[0] = g.cx1, s_norm[1] = g.cy1, s_norm[2] = g.cx2, s_norm[3] = g.cy2;
            __syncthreads();
        } else if (g.centred) {
            double c1x = 0, c1y = 0, c2x = 0, c2y = 0;
            for (uint32_t base = 0; base < n; base += kStatsChunk) {
                const uint32_t i = base + threadIdx.x;
                if (i < n) {
                    s_terms[threadIdx.x] = a_raw[2 * (size_t)i];
                    s_terms[kStatsChunk + threadIdx.x] = a_raw[2 * (size_t)i + 1];
                    s_terms[2 * kStatsChunk + threadIdx.x] = b_raw[2 * (size_t)i];
                    s_terms[3 * kStatsChunk + threadIdx.x] = b_raw[2 * (size_t)i + 1];
                }
                __syncthreads();
                if (adder) {
                    const int count = (int)(n - base < (uint32_t)kStatsChunk ? n - base : (uint32_t)kStatsChunk);
#pragma unroll 8
                    for (int k = 0; k < count; ++k) { // four sums, each in index order
                        c1x += s_terms[k];
                        c1y += s_terms[kStatsChunk + k];
                        c2x += s_terms[2 * kStatsChunk + k];
                        c2y += s_terms[3 * kStatsChunk + k];
                    }
                }
                __syncthreads();
            }
            if (threadIdx.x == 0) {
                s_norm[0] = c1x / g.n_as_double, s_norm[1] = c1y / g.n_as_double;
                s_norm[2] = c2x / g.n_as_double, s_norm[3] = c2y / g.n_as_double;
            }
            __syncthreads();
        }
        const double c1x = s_norm[0], c1y = s_norm[1], c2x = s_norm[2], c2y = s_norm[3];
        double scale = 0.0;
        for (uint32_t base = 0; base < n; base += kStatsChunk) {
            const uint32_t i = base + threadIdx.x;
            if (i < n) {
                double a0 = a_raw[2 * (size_t)i], a1 = a_raw[2 * (size_t)i + 1];
                double b0 = b_raw[2 * (size_t)i], b1 = b_raw[2 * (size_t)i + 1];
                if (g.centred || about)
                    a0 -= c1x, a1 -= c1y, b0 -= c2x, b1 -= c2y;
                s_terms[2 * threadIdx.x] = sqrt(a0 * a0 + a1 * a1);
                s_terms[2 * threadIdx.x + 1] = sqrt(b0 * b0 + b1 * b1);
            }
            __syncthreads();
            if (adder) {
                const int count = 2 * (int)(n - base < (uint32_t)kStatsChunk ? n - base : (uint32_t)kStatsChunk);
#pragma unroll 8
                for (int k = 0; k < count; ++k) // scale += |a_k|; scale += |b_k|, correspondence after correspondence
                    scale += s_terms[k];
            }
            __syncthreads();
        }
        if (threadIdx.x == 0)
            s_norm[4] = scale / g.scale_divisor;
    }
    __syncthreads();
    double m = 0.0;
    if (g.norm == 3) { // max |x * scale|, max |y * scale| of the block make_problem would have written (NaN propagates)
        const double scale = s_norm[4];
        for (uint32_t i = threadIdx.x; i < n; i += 256) {
            take_abs(m, a_raw[2 * (size_t)i] * scale);
            take_abs(m, a_raw[2 * (size_t)i + 1] * scale);
        }
    } else if (g.bound) {
        double cx1 = g.cx1, cy1 = g.cy1, fx1 = g.fx1, fy1 = g.fy1, cx2 = g.cx2, cy2 = g.cy2, fx2 = g.fx2, fy2 = g.fy2;
        if (g.bound == 3) { // (x - centroid) / scale; the host subtracts 0.0 when the points are not centred
            cx1 = s_norm[0], cy1 = s_norm[1], cx2 = s_norm[2], cy2 = s_norm[3];
            fx1 = fy1 = fx2 = fy2 = s_norm[4];
        }
        for (uint32_t i = threadIdx.x; i < n; i += 256) {
            take_abs(m, (a_raw[2 * (size_t)i] - cx1) / fx1);
            take_abs(m, (a_raw[2 * (size_t)i + 1] - cy1) / fy1);
            if (g.bound != 1) {
                take_abs(m, (b_raw[2 * (size_t)i] - cx2) / fx2);
                take_abs(m, (b_raw[2 * (size_t)i + 1] - cy2) / fy2);
            }
        }
    }
    const unsigned long long bits = wave_max_bits(m);
    if (lane == 0 && bits)
        atomicMax(&s_max, bits);
    __syncthreads();
    if (threadIdx.x == 0) {
        const bool nm = g.norm != 0;
        out->c1x = nm ? s_norm[0] : 0.0, out->c1y = nm ? s_norm[1] : 0.0;
        out->c2x = nm ? s_norm[2] : 0.0, out->c2y = nm ? s_norm[3] : 0.0;
        out->scale = nm ? s_norm[4] : 0.0;
        out->absmax = __longlong_as_double((long long)s_max);
        out->reserved[0] = out->reserved[1] = 0.0;
    }
}
__global__ __launch_bounds__(256) void k_point_stats(const double *__restrict__ a_raw, const double *__restrict__ b_raw, uint32_t n,
                                                     PointStatsArgs g, PointStatsRecord *__restrict__ out) {
    point_stats_body(a_raw, b_raw, n, g, out);
}
// One workgroup per member of a group (blockIdx.z); a member the host has no pass for (n == 0 in the table) gets no work and
// no record.  n and the arguments are the same for the whole workgroup, so are the body's barriers.
__global__ __launch_bounds__(256) void k_point_stats_g(const PointStatsGroupArgs *tab) {
    const PointStatsGroupArgs &in = tab[blockIdx.z];
    if (in.n == 0)
        return;
    point_stats_body(as_global(in.a_raw), as_global(in.b_raw), in.n, in.args, as_global(in.out));
}

// The un-distortion stage between two blocks of the caller's device memory: row i of the source through the ingest loader,
// camera_unproject, and k_undistort's expression (pipeline.hip; the same build flags) into columns 0 and 1 of row i of the
// destination - the host entry point's bits.  Both elements of the row are read before either is written: a destination that IS
// the source (same address, same stride, fp64) is served in place; the driver refuses every other overlap.
__device__ __forceinline__ void undistort_row(const IngestSrc &src, const CameraParams &cam, double fx, double fy, double cx, double cy,
                                              uint32_t i, double *out, int64_t out_stride) {
    const size_t row = (size_t)i * (size_t)src.row_stride;
    const double px = ingest_load(src.data, src.f32, row), py = ingest_load(src.data, src.f32, row + 1);
    double u, v;
    camera_unproject(cam, px, py, u, v);
    double *o = as_global(out) + (size_t)i * (size_t)out_stride;
    o[0] = fx * u + cx;
    o[1] = fy * v + cy;
}
__global__ __launch_bounds__(256) void k_undistort_dev(UndistortDevArgs in) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= in.n)
        return;
    undistort_row(in.src, in.cam, in.fx, in.fy, in.cx, in.cy, i, in.out, in.out_stride);
}
// ... of every member of a call (blockIdx.z, k_ingest_g's shape): blocks beyond a member's rows return, a member with n == 0 (an
// empty or refused item) does no work.  (in.cam, not a copy: the parameter array is indexed at run time, see k_prepare_g.)
__global__ __launch_bounds__(256) void k_undistort_dev_g(const UndistortDevArgs *tab) {
    const UndistortDevArgs &in = tab[blockIdx.z];
    const uint32_t n = in.n;
    if (blockIdx.x * 256u >= n)
        return;
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n)
        return;
    undistort_row(in.src, in.cam, in.fx, in.fy, in.cx, in.cy, i, in.out, in.out_stride);
}

// Zero flags in the caller's mask destinations (pl_estimate_dev_masked / _batch_dev_masked), in front of the runs that write the
// inliers' flags: one thread per row, one plain byte store.
__global__ __launch_bounds__(256) void k_mask_fill_g(const MaskFillArgs *tab) {
    const MaskFillArgs &in = tab[blockIdx.z];
    const uint32_t n = in.n;
    if (blockIdx.x * 256u >= n)
        return;
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n)
        return;
    as_global(in.data)[(size_t)i * (size_t)in.stride] = 0;
}
hipError_t launch_mask_fill_g(const MaskFillArgs *tab, uint32_t G, uint32_t max_n, hipStream_t stream) {
    constexpr uint32_t kMembersPerLaunch = 32768; // (a grid's z extent ends at 65535)
    for (uint32_t at = 0; at < G && max_n; at += kMembersPerLaunch) {
        k_mask_fill_g<<<dim3((max_n + 255) / 256, 1, G - at < kMembersPerLaunch ? G - at : kMembersPerLaunch), dim3(256), 0, stream>>>(tab + at);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess)
            return e;
    }
    return hipSuccess;
}

hipError_t launch_undistort_dev(const UndistortDevArgs &args, hipStream_t stream) {
    if (args.n == 0)
        return hipSuccess;
    k_undistort_dev<<<dim3((args.n + 255) / 256), dim3(256), 0, stream>>>(args);
    return hipGetLastError();
}
hipError_t launch_undistort_dev_g(const UndistortDevArgs *tab, uint32_t G, uint32_t max_n, hipStream_t stream) {
    constexpr uint32_t kMembersPerLaunch = 32768; // (a grid's z extent ends at 65535)
    for (uint32_t at = 0; at < G && max_n; at += kMembersPerLaunch) {
        k_undistort_dev_g<<<dim3((max_n + 255) / 256, 1, G - at < kMembersPerLaunch ? G - at : kMembersPerLaunch), dim3(256), 0, stream>>>(tab + at);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess)
            return e;
    }
    return hipSuccess;
}
hipError_t launch_ingest(const IngestSrc &a, const IngestSrc &b, uint32_t n, double *out_a, double *out_b, hipStream_t stream) {
    if (n == 0 || (!out_a && !out_b))
        return hipSuccess;
    k_ingest<<<dim3((n + 255) / 256), dim3(256), 0, stream>>>(a, b, n, out_a, out_b);
    return hipGetLastError();
}
hipError_t launch_ingest_g(const IngestGroupArgs *tab, uint32_t G, uint32_t max_n, hipStream_t stream) {
    if (G == 0 || max_n == 0)
        return hipSuccess;
    k_ingest_g<<<dim3((max_n + 255) / 256, 1, G), dim3(256), 0, stream>>>(tab);
    return hipGetLastError();
}
hipError_t launch_ingest_ranked(const IngestRankedArgs &args, hipStream_t stream) {
    if (args.n == 0)
        return hipSuccess;
    k_ingest_ranked<<<dim3((args.n + 255) / 256), dim3(256), 0, stream>>>(args);
    return hipGetLastError();
}
hipError_t launch_ingest_ranked_g(const IngestRankedArgs *tab, uint32_t G, uint32_t max_n, hipStream_t stream) {
    constexpr uint32_t kMembersPerLaunch = 32768; // (a grid's z extent ends at 65535)
    for (uint32_t at = 0; at < G && max_n; at += kMembersPerLaunch) {
        k_ingest_ranked_g<<<dim3((max_n + 255) / 256, 1, G - at < kMembersPerLaunch ? G - at : kMembersPerLaunch), dim3(256), 0, stream>>>(tab + at);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess)
            return e;
    }
    return hipSuccess;
}
hipError_t launch_point_stats_g(const PointStatsGroupArgs *tab, uint32_t G, hipStream_t stream) {
    if (G == 0)
        return hipSuccess;
    k_point_stats_g<<<dim3(1, 1, G), dim3(256), 0, stream>>>(tab);
    return hipGetLastError();
}
hipError_t launch_ingest_soa(const IngestSrc &a, const IngestSrc &b, uint32_t n, int b_in_max, double *soa,
                             unsigned long long *absmax_bits, hipStream_t stream, double scale_a) {
    if (n == 0)
        return hipSuccess;
    k_ingest_soa<<<dim3((n + 255) / 256), dim3(256), 0, stream>>>(a, b, n, b_in_max, scale_a, soa, absmax_bits);
    return hipGetLastError();
}
hipError_t launch_point_stats(const double *a_raw, const double *b_raw, uint32_t n, const PointStatsArgs &args, PointStatsRecord *out,
                              hipStream_t stream) {
    if (n == 0)
        return hipSuccess;
    k_point_stats<<<dim3(1), dim3(256), 0, stream>>>(a_raw, b_raw, n, args, out);
    return hipGetLastError();
}

} // namespace pl
