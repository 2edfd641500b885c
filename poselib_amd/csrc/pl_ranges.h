// poselib_amd — byte ranges of strided rows in the caller's device memory: the arithmetic behind the descriptor checks of the
// entry points that WRITE there (pl_undistort_points_dev, driver_dev.inc).  Plain host code without a HIP dependency, so that a
// stand-alone program can run it under a sanitizer (tests/hostcheck_device_results).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace pl {

// Bytes from the first element of row 0 to the end of the last used element of row n - 1: ((n - 1) * row_stride + cols) * elt.
// false: n == 0 (no bytes; *bytes = 0), a stride or width below 1, or a product that does not fit 64 bits.
inline bool rows_span_bytes(size_t n, int64_t row_stride, int cols, size_t elt, uint64_t *bytes) {
    *bytes = 0;
    if (n == 0 || row_stride < 1 || cols < 1 || elt == 0)
        return false;
    uint64_t v;
    if (__builtin_mul_overflow((uint64_t)(n - 1), (uint64_t)row_stride, &v) || __builtin_add_overflow(v, (uint64_t)cols, &v) ||
        __builtin_mul_overflow(v, (uint64_t)elt, &v))
        return false;
    *bytes = v;
    return true;
}

// [at, at + bytes) lies inside [lo, lo + size); an empty range lies inside anything
inline bool range_inside(uint64_t at, uint64_t bytes, uint64_t lo, uint64_t size) {
    if (bytes == 0)
        return true;
    return at >= lo && at - lo <= size && bytes <= size - (at - lo);
}

// [a, a + a_bytes) and [b, b + b_bytes) share a byte.  Ranges that touch do not; an empty range overlaps nothing; a range that
// would wrap past 2^64 is taken to reach the end of the address space.
inline bool ranges_overlap(uint64_t a, uint64_t a_bytes, uint64_t b, uint64_t b_bytes) {
    if (a_bytes == 0 || b_bytes == 0)
        return false;
    const uint64_t a_last = a_bytes - 1 > UINT64_MAX - a ? UINT64_MAX : a + (a_bytes - 1);
    const uint64_t b_last = b_bytes - 1 > UINT64_MAX - b ? UINT64_MAX : b + (b_bytes - 1);
    return a <= b_last && b <= a_last;
}

} // namespace pl
