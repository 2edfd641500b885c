// Stand-alone check of poselib_amd/csrc/pl_ranges.h - the extent and overlap arithmetic of pl_undistort_points_dev's descriptor
// checks - built with -fsanitize=address,undefined (see the Makefile): the edge cases, and every small case against a byte map.
#include "../../poselib_amd/csrc/pl_ranges.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace pl;

static int failures = 0;
#define CHECK(cond)                                                                                                    \
    do {                                                                                                               \
        if (!(cond)) {                                                                                                 \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);                                                      \
            ++failures;                                                                                                \
        }                                                                                                              \
    } while (0)

int main() {
    uint64_t bytes = 7;
    // n == 0: no bytes, whatever the rest says
    CHECK(!rows_span_bytes(0, 2, 2, 8, &bytes) && bytes == 0);
    CHECK(!rows_span_bytes(0, -5, 2, 8, &bytes) && bytes == 0);
    // one row, many rows, a wide stride
    CHECK(rows_span_bytes(1, 2, 2, 8, &bytes) && bytes == 16);
    CHECK(rows_span_bytes(1, 1 << 28, 2, 8, &bytes) && bytes == 16);
    CHECK(rows_span_bytes(10, 2, 2, 8, &bytes) && bytes == 160);
    CHECK(rows_span_bytes(10, 5, 2, 4, &bytes) && bytes == (9 * 5 + 2) * 4);
    CHECK(rows_span_bytes(0x7fffffffu, (int64_t)1 << 28, 2, 8, &bytes) && bytes == ((uint64_t)0x7ffffffeu * ((uint64_t)1 << 28) + 2) * 8);
    // a stride, a width or an element size that is none
    CHECK(!rows_span_bytes(10, 0, 2, 8, &bytes) && bytes == 0);
    CHECK(!rows_span_bytes(10, -3, 2, 8, &bytes));
    CHECK(!rows_span_bytes(10, 2, 0, 8, &bytes));
    CHECK(!rows_span_bytes(10, 2, 2, 0, &bytes));
    // stride x n beyond 64 bits: the product, the sum and the scaling by the element size
    CHECK(!rows_span_bytes((size_t)1 << 40, (int64_t)1 << 40, 2, 8, &bytes) && bytes == 0);
    CHECK(!rows_span_bytes(SIZE_MAX, INT64_MAX, 2, 8, &bytes));
    CHECK(!rows_span_bytes(2, INT64_MAX, 2, 8, &bytes));
    CHECK(!rows_span_bytes(((size_t)1 << 32) + 1, (int64_t)1 << 29, 2, 8, &bytes)); // 2^61 + 2 elements fit, times 8 does not
    CHECK(rows_span_bytes((size_t)1 << 32, (int64_t)1 << 29, 2, 8, &bytes) && bytes == ((((uint64_t)1 << 32) - 1) * ((uint64_t)1 << 29) + 2) * 8);
    CHECK(rows_span_bytes(((size_t)1 << 32) + 1, (int64_t)1 << 28, 2, 8, &bytes) && bytes == (((uint64_t)1 << 60) + 2) * 8);

    // ranges that touch do not overlap; identical ranges do; an empty range overlaps nothing
    CHECK(!ranges_overlap(1000, 160, 1160, 160));
    CHECK(!ranges_overlap(1160, 160, 1000, 160));
    CHECK(ranges_overlap(1000, 160, 1159, 1));
    CHECK(ranges_overlap(1000, 160, 1000, 160));
    CHECK(ranges_overlap(1000, 160, 1080, 160) && ranges_overlap(1080, 160, 1000, 160));
    CHECK(ranges_overlap(1000, 160, 1040, 8) && ranges_overlap(1040, 8, 1000, 160)); // one inside the other
    CHECK(!ranges_overlap(1000, 0, 1000, 160) && !ranges_overlap(1000, 160, 1000, 0) && !ranges_overlap(1000, 0, 1000, 0));
    // at the top of the address space
    CHECK(!ranges_overlap(UINT64_MAX - 15, 16, UINT64_MAX - 31, 16));
    CHECK(ranges_overlap(UINT64_MAX - 15, 16, UINT64_MAX - 16, 2));
    CHECK(ranges_overlap(UINT64_MAX - 15, 1000, UINT64_MAX, 1)); // (a range that would wrap reaches the end)
    CHECK(!ranges_overlap(UINT64_MAX - 15, 1000, 0, 16));
    CHECK(ranges_overlap(0, UINT64_MAX, UINT64_MAX - 1, 1) && !ranges_overlap(0, UINT64_MAX, UINT64_MAX, 1));

    // inside an allocation
    CHECK(range_inside(1000, 160, 1000, 160) && range_inside(1000, 0, 5000, 1));
    CHECK(!range_inside(1000, 161, 1000, 160) && !range_inside(999, 16, 1000, 160) && !range_inside(1152, 16, 1000, 160));
    CHECK(range_inside(1144, 16, 1000, 160) && range_inside(1160, 0, 1000, 160) && !range_inside(1161, 1, 1000, 160));
    CHECK(!range_inside(UINT64_MAX - 7, 16, UINT64_MAX - 100, 101) && range_inside(UINT64_MAX - 7, 8, UINT64_MAX - 100, 101));

    // every small case against a byte map: two strided row sets in a window of 96 bytes
    for (size_t n = 0; n <= 4; ++n)
        for (int64_t sa = 2; sa <= 4; ++sa)
            for (int64_t sb = 2; sb <= 4; ++sb)
                for (uint64_t a = 0; a < 24; a += 4)
                    for (uint64_t b = 0; b < 24; b += 4) {
                        uint64_t la = 0, lb = 0;
                        const bool oka = rows_span_bytes(n, sa, 2, 4, &la), okb = rows_span_bytes(n, sb, 2, 4, &lb);
                        CHECK(oka == (n > 0) && okb == (n > 0));
                        std::vector<unsigned char> map(96, 0); // (the sanitizer watches the map's bounds as well)
                        for (uint64_t k = 0; k < la; ++k)
                            map[a + k] |= 1;
                        bool shared = false;
                        for (uint64_t k = 0; k < lb; ++k)
                            shared = shared || (map[b + k] & 1);
                        CHECK(ranges_overlap(a, la, b, lb) == shared);
                        CHECK(range_inside(a, la, 0, 96));
                    }
    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("ranges_check ok\n");
    return 0;
}
