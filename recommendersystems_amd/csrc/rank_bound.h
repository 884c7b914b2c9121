// The score bound that prunes the body rows of a batch's last step ("Pruning the body").  For one tile of seeds
// with thresholds tau[s] > 0 and a source row u with z[u][s] >= 0,
//     m[u] = max over the tile's real slots s of z[u][s] / tau[s], rounded UP to float (bound_term, bound_max)
// and a body row whose float sum F of m[u] over its in-list passes bound_prunes(F, in-degree) reaches tau for no seed of the
// tile: k_spmm_select would compute it and drop it.  Why the test is safe for a row of d <= BOUND_MAX_DEG in-links:
//   * the double score k_spmm_select forms in list order is S <= E (1 + d 2^-53), E the exact sum of the row's z[u][s];
//   * z / tau divided in double is >= the exact ratio x (1 - 2^-53), and bound_term never lies below that double;
//   * the float sum of d such terms, in any order, is F >= (exact sum of the terms) x (1 - d 2^-24); terms so small that a float
//     add flushes them lose at most d 2^-126 in all;
//   * so S >= tau for some s gives exact sum of m >= (1 - 2^-53) / (1 + d 2^-53) and F >= 1 - (d + 1) 2^-24 - 2^-50 > 1 - 2^-11
//     for d <= 2^12, and F x BOUND_SLACK, itself rounded (x (1 - 2^-24)), is >= 1: the row is kept.  Ties (S == tau) are kept too.
// Rows of more than BOUND_MAX_DEG in-links are never tested.  Plain C++17 without HIP in the host build, so that
// tests/cpp/rank_bound_check.cpp checks the rounding on the host.
#pragma once

#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define RWR_BOUND_HD __host__ __device__
#else
#define RWR_BOUND_HD
#endif

namespace rwr {

constexpr int32_t BOUND_MAX_DEG = 1 << 12;                 // in-links of a row the test applies to
constexpr float BOUND_SLACK = 1.0f + 1.0f / 2048.0f;       // 1 + 2^-11: covers (BOUND_MAX_DEG + 1) 2^-24 twice over

// q >= 0 (or +inf) as a float that is not below it
RWR_BOUND_HD inline float bound_round_up(double q)
{
    float f = (float)q;                                    // to nearest: at most one float below q
    if ((double)f < q) {                                   // (f is finite here: +inf is below nothing)
        uint32_t b;
        memcpy(&b, &f, 4);
        ++b;                                               // the next float up of a finite f >= +0.0 (FLT_MAX -> +inf)
        memcpy(&f, &b, 4);
    }
    return f;
}

// one slot's term of m[u]: z >= 0, tau > 0
RWR_BOUND_HD inline float bound_term(double z, double tau) { return bound_round_up(z / tau); }

// true: no seed of the tile reaches its threshold in a row of `deg` in-links whose float sum of m[u] is `sum`
RWR_BOUND_HD inline bool bound_prunes(float sum, int64_t deg) { return deg <= BOUND_MAX_DEG && sum * BOUND_SLACK < 1.0f; }

}  // namespace rwr
