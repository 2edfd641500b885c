// poselib_amd — ranking a matcher's confidences on the device (gfx950): which rows of an item are correspondences at all, and in
// which order PROSAC should meet them.  Like ingest.hip this sits IN FRONT of the existing preparation: the permutation it leaves in
// device memory is what k_ingest_ranked (ingest.hip) copies rows by, and from there on nothing knows that scores were involved.
//
// The rule (include/poselib_amd.h): row i is kept iff score[i] >= min_score - a NaN score never is -, kept rows go in descending
// score, equal scores (-0.0 == 0.0) in ascending row index.  Both dtypes take one route: an fp32 score is widened (exactly) and every
// row becomes the pair
//     key  = the bits of the score, +0.0 for -0.0, mapped so that unsigned ascending order is descending score; all ones for a
//            dropped row (no kept row has that key: it would be a NaN)
//     row  = the row index
// whose lexicographic order is total - no two pairs are equal -, so the permutation is the same whatever computes it:
//   k_rank_tile    one workgroup per tile of T rows: keys from global memory, a bitonic network over (key, row) in LDS.  A member of
//                  at most T rows is finished here: order[] and the kept count are written from LDS.
//   k_rank_merge   larger members: sorted runs of T, 2T, ... rows are merged pairwise through global memory, one thread per row - its
//                  place is its offset in its own run plus the number of rows of the partner run that go before it (a binary search;
//                  exact because the order is total).  log2(ceil(n / T)) passes.
//   k_rank_finish  ... and order[] / the kept count from the last pass's side
// Each has a single form (arguments as kernel arguments) and a grouped one (member = blockIdx.z, arguments from a device-visible
// table), one body.  No atomics, nothing to zero, no scratch beyond the two sides of the merge.
#include "pl_kernels.h"
#include "pl_global.h"

namespace pl {

namespace {

constexpr unsigned long long kDropped = ~0ull;
constexpr int kSmallTile = 1024, kSmallThreads = 256; // 12 KiB of LDS: several workgroups per CU for a batch of small members
constexpr int kLargeTile = 8192, kLargeThreads = 1024; // 96 KiB of the 160 KiB
constexpr int kMergeThreads = 256;

__device__ __forceinline__ unsigned long long rank_key(const RankSrc &s, size_t row) {
    const size_t at = row * (size_t)s.stride;
    const double v = s.f32 ? (double)as_global(static_cast<const float *>(s.data))[at] : as_global(static_cast<const double *>(s.data))[at];
    if (!(v >= s.min_score)) // (IEEE: false for a NaN score)
        return kDropped;
    const unsigned long long bits = v == 0.0 ? 0ull : (unsigned long long)__double_as_longlong(v);
    const unsigned long long ascending = (bits >> 63) ? ~bits : (bits | 0x8000000000000000ull);
    return ~ascending;
}
__device__ __forceinline__ bool goes_before(unsigned long long ka, uint32_t ra, unsigned long long kb, uint32_t rb) {
    return ka < kb || (ka == kb && ra < rb);
}
__device__ __forceinline__ RankArgs globalised(RankArgs g) {
    g.keys[0] = as_global(g.keys[0]), g.keys[1] = as_global(g.keys[1]);
    g.rows[0] = as_global(g.rows[0]), g.rows[1] = as_global(g.rows[1]);
    g.order = as_global(g.order);
    g.kept = as_global(g.kept);
    return g;
}

// order[] and the kept count from a sorted sequence: the kept rows are its head, position j speaks for itself
__device__ __forceinline__ void rank_emit(const RankArgs &g, uint32_t j, unsigned long long key, uint32_t row, bool last,
                                          unsigned long long next_key) {
    if (key != kDropped) {
        g.order[j] = row;
        if (last || next_key == kDropped)
            *g.kept = j + 1;
    } else if (j == 0) {
        *g.kept = 0;
    }
}

template <int T, int THREADS> __device__ __forceinline__ void rank_tile_body(const RankArgs &g) {
    __shared__ unsigned long long s_key[T];
    __shared__ uint32_t s_row[T];
    const uint32_t n = g.n;
    if (n == 0) {
        if (blockIdx.x == 0 && threadIdx.x == 0)
            *g.kept = 0;
        return;
    }
    if ((size_t)blockIdx.x * T >= n) // (n, and with it every loop bound and barrier below, is the same for the whole workgroup)
        return;
    const uint32_t base = blockIdx.x * (uint32_t)T;
    const uint32_t valid = n - base < (uint32_t)T ? n - base : (uint32_t)T;
    uint32_t P = 2; // the network's size: a power of two; the padding goes behind every row of the tile
    while (P < valid)
        P <<= 1;
    for (uint32_t i = threadIdx.x; i < P; i += THREADS) {
        s_key[i] = i < valid ? rank_key(g.s, (size_t)base + i) : kDropped;
        s_row[i] = i < valid ? base + i : 0xffffffffu;
    }
    __syncthreads();
    for (uint32_t k = 2; k <= P; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = threadIdx.x; t < (P >> 1); t += THREADS) {
                const uint32_t lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                const unsigned long long ka = s_key[lo], kb = s_key[hi];
                const uint32_t ra = s_row[lo], rb = s_row[hi];
                const bool ascending = (lo & k) == 0;
                if (goes_before(kb, rb, ka, ra) == ascending) {
                    s_key[lo] = kb, s_key[hi] = ka;
                    s_row[lo] = rb, s_row[hi] = ra;
                }
            }
            __syncthreads();
        }
    if (n <= (uint32_t)T) { // the whole member: done
        for (uint32_t i = threadIdx.x; i < valid; i += THREADS)
            rank_emit(g, i, s_key[i], s_row[i], i + 1 == valid, i + 1 < valid ? s_key[i + 1] : kDropped);
        return;
    }
    for (uint32_t i = threadIdx.x; i < valid; i += THREADS) {
        g.keys[0][(size_t)base + i] = s_key[i];
        g.rows[0][(size_t)base + i] = s_row[i];
    }
}

// The two sides of a member's merge passes, picked by value: an index into keys[] / rows[] that the compiler cannot fold puts the
// argument record into scratch, and a pointer that comes back from scratch is a flat address again.
struct RankSides {
    const unsigned long long *kin;
    const uint32_t *rin;
    unsigned long long *kout;
    uint32_t *rout;
};
__device__ __forceinline__ RankSides rank_sides(const RankArgs &g, int src) {
    RankSides s;
    s.kin = as_global(src ? g.keys[1] : g.keys[0]), s.rin = as_global(src ? g.rows[1] : g.rows[0]);
    s.kout = as_global(src ? g.keys[0] : g.keys[1]), s.rout = as_global(src ? g.rows[0] : g.rows[1]);
    return s;
}

// runs of `run` rows on side `src`, pairwise -> runs of 2 * run rows on the other side (a last run without a partner is copied)
__device__ __forceinline__ void rank_merge_body(const RankArgs &g, uint32_t tile, uint32_t run, int src) {
    const uint32_t n = g.n;
    if (n <= tile || (size_t)blockIdx.x * kMergeThreads >= n)
        return;
    const uint32_t j = blockIdx.x * (uint32_t)kMergeThreads + threadIdx.x;
    if (j >= n)
        return;
    const RankSides side = rank_sides(g, src);
    const unsigned long long *__restrict__ kin = side.kin;
    const uint32_t *__restrict__ rin = side.rin;
    const unsigned long long key = kin[j];
    const uint32_t row = rin[j];
    const uint32_t r = j / run;
    const size_t own = (size_t)r * run, partner = (size_t)(r ^ 1u) * run, pair = (size_t)(r & ~1u) * run;
    size_t lo = partner, hi = partner;
    if (partner < n)
        hi = partner + run < n ? partner + run : n;
    while (lo < hi) { // the first row of the partner run that does not go before this one
        const size_t mid = lo + ((hi - lo) >> 1);
        const unsigned long long km = kin[mid];
        if (km < key || (km == key && rin[mid] < row))
            lo = mid + 1;
        else
            hi = mid;
    }
    const size_t pos = pair + (j - own) + (partner < n ? lo - partner : 0);
    side.kout[pos] = key;
    side.rout[pos] = row;
}

__device__ __forceinline__ void rank_finish_body(const RankArgs &g, uint32_t tile, int src) {
    const uint32_t n = g.n;
    if (n <= tile || (size_t)blockIdx.x * kMergeThreads >= n)
        return;
    const uint32_t j = blockIdx.x * (uint32_t)kMergeThreads + threadIdx.x;
    if (j >= n)
        return;
    const RankSides side = rank_sides(g, src);
    RankArgs out = g;
    out.order = as_global(g.order), out.kept = as_global(g.kept);
    rank_emit(out, j, side.kin[j], side.rin[j], j + 1 == n, j + 1 < n ? side.kin[j + 1] : kDropped);
}

} // namespace

template <int T, int THREADS> __global__ __launch_bounds__(THREADS) void k_rank_tile(RankArgs g) { rank_tile_body<T, THREADS>(g); }
template <int T, int THREADS> __global__ __launch_bounds__(THREADS) void k_rank_tile_g(const RankArgs *tab) {
    rank_tile_body<T, THREADS>(globalised(tab[blockIdx.z]));
}
__global__ __launch_bounds__(kMergeThreads) void k_rank_merge(RankArgs g, uint32_t tile, uint32_t run, int src) {
    rank_merge_body(g, tile, run, src);
}
__global__ __launch_bounds__(kMergeThreads) void k_rank_merge_g(const RankArgs *tab, uint32_t tile, uint32_t run, int src) {
    rank_merge_body(tab[blockIdx.z], tile, run, src);
}
__global__ __launch_bounds__(kMergeThreads) void k_rank_finish(RankArgs g, uint32_t tile, int src) { rank_finish_body(g, tile, src); }
__global__ __launch_bounds__(kMergeThreads) void k_rank_finish_g(const RankArgs *tab, uint32_t tile, int src) {
    rank_finish_body(tab[blockIdx.z], tile, src);
}

uint32_t rank_tile(uint32_t max_n) { return max_n <= (uint32_t)kSmallTile ? (uint32_t)kSmallTile : (uint32_t)kLargeTile; }

namespace {
// the launch sequence of both forms: tab == null is the single form with `one`
hipError_t rank_sequence(const RankArgs *one, const RankArgs *tab, uint32_t G, uint32_t max_n, hipStream_t stream) {
    const uint32_t tile = rank_tile(max_n);
    const uint32_t tiles = max_n ? (max_n + tile - 1) / tile : 1;
    const dim3 tile_grid(tiles, 1, G);
    if (tile == (uint32_t)kSmallTile) {
        if (tab)
            k_rank_tile_g<kSmallTile, kSmallThreads><<<tile_grid, dim3(kSmallThreads), 0, stream>>>(tab);
        else
            k_rank_tile<kSmallTile, kSmallThreads><<<tile_grid, dim3(kSmallThreads), 0, stream>>>(*one);
    } else {
        if (tab)
            k_rank_tile_g<kLargeTile, kLargeThreads><<<tile_grid, dim3(kLargeThreads), 0, stream>>>(tab);
        else
            k_rank_tile<kLargeTile, kLargeThreads><<<tile_grid, dim3(kLargeThreads), 0, stream>>>(*one);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || max_n <= tile)
        return e;
    const dim3 row_grid((max_n + kMergeThreads - 1) / kMergeThreads, 1, G);
    int src = 0;
    for (uint64_t run = tile; run < max_n; run <<= 1, src ^= 1) {
        if (tab)
            k_rank_merge_g<<<row_grid, dim3(kMergeThreads), 0, stream>>>(tab, tile, (uint32_t)run, src);
        else
            k_rank_merge<<<row_grid, dim3(kMergeThreads), 0, stream>>>(*one, tile, (uint32_t)run, src);
        e = hipGetLastError();
        if (e != hipSuccess)
            return e;
    }
    if (tab)
        k_rank_finish_g<<<row_grid, dim3(kMergeThreads), 0, stream>>>(tab, tile, src);
    else
        k_rank_finish<<<row_grid, dim3(kMergeThreads), 0, stream>>>(*one, tile, src);
    return hipGetLastError();
}
} // namespace

hipError_t launch_rank(const RankArgs &args, hipStream_t stream) { return rank_sequence(&args, nullptr, 1, args.n, stream); }
hipError_t launch_rank_g(const RankArgs *tab, uint32_t G, uint32_t max_n, hipStream_t stream) {
    constexpr uint32_t kMembersPerLaunch = 32768; // (a grid's z extent ends at 65535)
    for (uint32_t at = 0; at < G; at += kMembersPerLaunch) {
        const hipError_t e = rank_sequence(nullptr, tab + at, G - at < kMembersPerLaunch ? G - at : kMembersPerLaunch, max_n, stream);
        if (e != hipSuccess)
            return e;
    }
    return hipSuccess;
}

} // namespace pl
