// Host check of recommendersystems_amd/csrc/rank_bound.h (tests/test_rank_bound.py): the float bound of a row never falls below
// its in-order double score divided by the threshold, so a row that reaches the threshold is never pruned; ties are kept.
#include "rank_bound.h"

#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

using namespace rwr;

static int failures = 0;
#define CHECK(c, ...) do { if (!(c)) { ++failures; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

int main()
{
    std::mt19937_64 rng(12345);
    std::uniform_real_distribution<double> uni(0.0, 1.0);
    // bound_round_up: never below its argument, at most one float above the nearest
    const double probes[] = {0.0, 4.9e-324, 1e-310, 1.17549435e-38, 1e-45, 0.1, 1.0, 1.0 + 1e-12, 3.4028234e38, 3.5e38, 1e300, INFINITY};
    for (double q : probes) {
        const float f = bound_round_up(q);
        CHECK((double)f >= q, "round_up(%g) = %g", q, (double)f);
        CHECK(f == (float)q || f == std::nextafterf((float)q, INFINITY), "round_up(%g) too far", q);
    }
    for (int i = 0; i < 2000000; ++i) {
        const double q = std::ldexp(uni(rng), (int)(rng() % 300) - 200);
        CHECK((double)bound_round_up(q) >= q, "round_up(%a)", q);
    }
    // rows: random non-negative z over many magnitudes, in-degrees up to the cap; thresholds at, just below and just above
    // the row's own score, and at random
    long pruned = 0, kept = 0;
    for (int trial = 0; trial < 60000; ++trial) {
        const int d = trial % 7 == 0 ? 1 + (int)(rng() % BOUND_MAX_DEG) : 1 + (int)(rng() % 40);
        const int spread = (int)(rng() % 60);
        std::vector<double> z(d);
        double score = 0.0;
        for (int i = 0; i < d; ++i) {
            z[i] = (rng() % 8 == 0) ? 0.0 : std::ldexp(uni(rng), -(int)(rng() % (spread + 1)));
            score += z[i];                                   // the list-order double sum of k_spmm_select
        }
        if (!(score > 0.0)) continue;
        const double taus[] = {score, std::nextafter(score, 0.0), std::nextafter(score, INFINITY), score * (1.0 + 1e-7),
                               score * (1.0 + 3e-4), score * 1.001, score * 2.0, score * uni(rng), score * (1.0 + uni(rng))};
        for (double tau : taus) {
            float sum = 0.0f;
            for (int i = 0; i < d; ++i) {
                const float m = bound_term(z[i], tau);
                CHECK((double)m >= z[i] / tau, "term below the ratio");
                sum += m;
            }
            const bool p = bound_prunes(sum, d);
            if (score >= tau) CHECK(!p, "a row of %d links that reaches tau was pruned (score/tau - 1 = %g)", d, score / tau - 1.0);
            // the float bound against the double ratio itself
            CHECK((double)sum * (double)BOUND_SLACK >= score / tau, "bound %g below score / tau %g (d = %d)", (double)sum, score / tau, d);
            p ? ++pruned : ++kept;
        }
    }
    CHECK(pruned > 100000 && kept > 100000, "the sweep is lopsided: %ld pruned, %ld kept", pruned, kept);
    // beyond the cap nothing is pruned; infinities and the empty row
    CHECK(!bound_prunes(0.0f, (int64_t)BOUND_MAX_DEG + 1), "a row beyond the cap was pruned");
    CHECK(bound_prunes(0.0f, 0), "an empty row with a positive threshold was kept");
    CHECK(!bound_prunes(INFINITY, 3), "an infinite bound was pruned");
    CHECK(!bound_prunes(1.0f, 1) && !bound_prunes(std::nextafterf(1.0f, 0.0f), 1), "a bound at 1 was pruned");
    CHECK(bound_term(1.0, 1.0) == 1.0f && bound_term(0.0, 5.0) == 0.0f, "exact ratios must stay exact");
    std::printf("%ld pruned, %ld kept\n%d failures\n", pruned, kept, failures);
    return failures ? 1 : 0;
}
