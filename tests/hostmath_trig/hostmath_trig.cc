// TEST-ONLY host compilation of pl_atan2 / pl_tan (poselib_amd/csrc/pl_libm.h) next to the host's own atan2 / tan, so that the
// CPU test-suite can compare them bit for bit on tens of millions of arguments, and so that the GPU tests can send the same
// arguments to the device.  Never used by the product.
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../poselib_amd/csrc/pl_libm.h"

using namespace pl;

namespace {
enum { FN_ATAN2 = 0, FN_TAN = 1 };
// the arguments of the tests' streams: (a, b) = (y, x) for atan2, (x, -) for tan
struct ArgStream {
    int fn;
    uint64_t s, i = 0;
    ArgStream(int fn_, uint64_t seed) : fn(fn_), s(seed * 0x9E3779B97F4A7C15ull + 88172645463325252ull) {}
    uint64_t rnd() {
        s ^= s << 13, s ^= s >> 7, s ^= s << 17;
        return s;
    }
    double unit() { return (double)(rnd() >> 11) / 9007199254740992.0; } // [0, 1)
    double logu(int emin, int emax) { return std::ldexp(unit() + 0.5, emin + (int)(rnd() % (uint64_t)(emax - emin + 1))); }
    void next(double &a, double &b) {
        const uint64_t k = i++;
        if (fn == FN_ATAN2) {
            const uint64_t r = rnd();
            const double sx = (r & 1) ? -1.0 : 1.0, sy = (r & 6) ? 1.0 : -1.0; // (the cameras' y = rho is positive: 3 of 4)
            switch (k % 5) {
            case 0: // log-uniform magnitudes, every ratio up to 2^+-120
                a = sy * logu(-60, 60), b = sx * logu(-60, 60);
                break;
            case 1: // what the fisheye projections send: rho in (0, 10), z in [-10, 10)
                a = unit() * 10 + 1e-8, b = unit() * 20 - 10;
                break;
            case 2: { // |y| / |x| near 1 and near 1 / 16 (the switches of the algorithm), any scale
                const double m = logu(-30, 30), e = std::ldexp(unit() - 0.5, -(int)(rnd() % 50));
                const double q = (r & 8) ? 1.0 : ((r & 16) ? 16.0 : 0.0625);
                a = sy * m, b = sx * m * q * (1.0 + e);
                break;
            }
            case 3: // the whole exponent range of normal numbers
                a = sy * logu(-1021, 1022), b = sx * logu(-1021, 1022);
                break;
            default: // ratios inside the table's range [1 / 16, 1], either way round
                a = sy * logu(-8, 8), b = sx * std::fabs(a) * (1.0 + 15.0 * unit());
                if (r & 32) {
                    const double t = a;
                    a = sy * std::fabs(b), b = sx * std::fabs(t);
                }
            }
        } else {
            b = 0.0;
            switch (k % 4) {
            case 0:
                a = unit() * 50 - 25;
                break;
            case 1: // what the un-projection sends
                a = unit() * 3.141592653589793;
                break;
            case 2:
                a = ((rnd() & 1) ? -1.0 : 1.0) * logu(-40, 4);
                break;
            default: { // towards the multiples of pi / 2
                const double n = (double)(rnd() % 16);
                a = n * 1.5707963267948966 + std::ldexp(2 * unit() - 1, -(int)(rnd() % 50));
                if (rnd() & 1)
                    a = -a;
            }
            }
        }
    }
};
bool same(double p, double q) { return std::memcmp(&p, &q, 8) == 0 || (p != p && q != q); }
} // namespace

extern "C" {

void ht_args(int fn, uint64_t seed, uint64_t count, double *a, double *b) {
    ArgStream g(fn, seed);
    for (uint64_t i = 0; i < count; ++i)
        g.next(a[i], b[i]);
}
// the host's libm: fn 0: atan2(a, b), fn 1: tan(a)
void ht_glibc(int fn, const double *a, const double *b, uint64_t n, double *out) {
    for (uint64_t i = 0; i < n; ++i)
        out[i] = fn == FN_ATAN2 ? std::atan2(a[i], b[i]) : std::tan(a[i]);
}
// pl_libm.h: fn 0: pl_atan2(a, b), fn 1: pl_tan(a)
void ht_pl(int fn, const double *a, const double *b, uint64_t n, double *out) {
    for (uint64_t i = 0; i < n; ++i)
        out[i] = fn == FN_ATAN2 ? pl_atan2(a[i], b[i]) : pl_tan(a[i]);
}
// number of arguments of the stream on which the two differ in any bit; bad[0 .. 1]: the first such pair
uint64_t ht_mismatches(int fn, uint64_t count, uint64_t seed, double *bad) {
    ArgStream g(fn, seed);
    uint64_t n = 0;
    for (uint64_t i = 0; i < count; ++i) {
        double a, b;
        g.next(a, b);
        const double mine = fn == FN_ATAN2 ? pl_atan2(a, b) : pl_tan(a);
        const double host = fn == FN_ATAN2 ? std::atan2(a, b) : std::tan(a);
        if (!same(mine, host)) {
            if (!n && bad)
                bad[0] = a, bad[1] = b;
            ++n;
        }
    }
    return n;
}
}
