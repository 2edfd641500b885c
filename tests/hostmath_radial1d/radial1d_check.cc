// TEST-ONLY stand-alone program: the host compilation of the 1D-radial solver, scorer, pre-filter and refiner (hostmath_radial1d.cc)
// under AddressSanitizer and UndefinedBehaviorSanitizer.  Reads a binary file of doubles - S, then S samples of x (5 x 2) and
// X (5 x 3); n, a pose (7), x (n x 2), X (n x 3), a threshold - runs the solver over the samples and score, pre-filter and one
// refinement over the scene, and prints a line of totals.  Exit status 0 = the sanitizers found nothing.
#include "hostmath_radial1d.cc"

#include <cstdio>
#include <vector>

int main(int argc, char **argv) {
    if (argc != 2)
        return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f)
        return 3;
    std::vector<double> in;
    double buf[256];
    size_t got;
    while ((got = std::fread(buf, sizeof(double), 256, f)) > 0)
        in.insert(in.end(), buf, buf + got);
    std::fclose(f);
    if (in.empty())
        return 3;
    size_t at = 0;
    const uint32_t S = (uint32_t)in[at++];
    if (in.size() < 1 + 25 * (size_t)S + 1)
        return 3;
    std::vector<double> xs(10 * (size_t)S), Xs(15 * (size_t)S);
    for (uint32_t s = 0; s < S; ++s) {
        for (int k = 0; k < 10; ++k)
            xs[10 * s + k] = in[at++];
        for (int k = 0; k < 15; ++k)
            Xs[15 * s + k] = in[at++];
    }
    std::vector<uint32_t> counts(S);
    std::vector<double> poses(28 * (size_t)S, 0.0);
    std::vector<uint8_t> nan(4 * (size_t)S, 0);
    rd_p5lp(xs.data(), Xs.data(), S, counts.data(), poses.data(), nan.data());
    unsigned long models = 0;
    for (uint32_t s = 0; s < S; ++s)
        models += counts[s];
    const uint32_t n = (uint32_t)in[at++];
    if (in.size() < at + 7 + 5 * (size_t)n + 1)
        return 3;
    double pose[7];
    for (int k = 0; k < 7; ++k)
        pose[k] = in[at++];
    const double *x = &in[at], *X = &in[at + 2 * (size_t)n];
    const double thr = in[at + 5 * (size_t)n];
    uint64_t count = 0;
    std::vector<uint8_t> mask(n), rej(n), inl(n);
    const double score = rd_score(pose, x, X, n, thr * thr, &count, mask.data());
    const int status = rd_prefilter(pose, x, X, n, thr * thr, rej.data(), inl.data());
    LMOptions opt;
    opt.max_iterations = 25, opt.loss_type = LOSS_TRUNCATED, opt.lambda_update = 0, opt.damping = 0, opt.loss_scale = thr;
    opt.gradient_tol = 1e-12, opt.step_tol = 1e-8, opt.relative_cost_tol = 1e-10;
    opt.initial_lambda = 1e-3, opt.min_lambda = 1e-10, opt.max_lambda = 1e10, opt.lambda_factor = 10.0;
    uint32_t iterations = 0;
    double costs[2];
    rd_refine(x, X, n, pose, &opt, nullptr, &iterations, costs);
    std::printf("models %lu score %.17g count %llu filter %d iterations %u cost %.17g\n", models, score, (unsigned long long)count, status,
                iterations, costs[1]);
    return 0;
}
