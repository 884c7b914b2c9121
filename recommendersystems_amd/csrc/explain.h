// Reasons for ranked entries (internal; explain.hip): one more optional stage of the ranked end, for the list
// destination only.  The group's lists are written by a row-carrying collect and sort-and-emit in the place of the stock
// select's last two launches -- order (score desc, id desc, row asc), the rows kept beside ids and scores -- and the reasons
// kernel then walks the in-list of every live entry over the previous ranks.
#pragma once
#include "explain_plan.h"
#include "iterate.h"

namespace rwr {

// The explanation of one call.  The object is declared before the driver's StreamsIdle (ranked_end.h's lifetime rule).
struct WhyEnd {
    int32_t n_why = 0;                     // in [0, WHY_MAX]
    int64_t T = 0;                         // steps of the walk: T <= 0 has no previous ranks and no reasons
    double c1 = 0.0;                       // 1 - d
    // the caller's tables (host): nodes and why_total may be nullptr, why_src / why_term with n_why == 0
    int32_t *nodes = nullptr, *why_src = nullptr;
    double *why_term = nullptr;
    int64_t *why_total = nullptr;

    bool reasons() const { return T > 0 && (n_why > 0 || why_total); }
    DevBuf<int32_t> d_row, d_src;          // K x top_n rows (-1: no entry), K x top_n x n_why sources (-1: unused)
    DevBuf<double> d_term;                 // ... their addends (+0.0: unused)
    DevBuf<int64_t> d_total;               // K x top_n counts of positive addends
};

// the call's tables, in their "unused" state
int32_t why_prepare(rwr_graph *g, WhyEnd &w, int32_t K, int32_t top_n, hipStream_t s);
// the ranking of a tile group over `rows` (nrows > 0): the stock levels, then the row-carrying collect and sort-and-emit
int32_t why_rank_group(rwr_graph *g, WhyEnd &w, int G, int tg, const int32_t *slot_k, int32_t top_n, const double *X, hipStream_t s,
                       const int32_t *rows, int32_t nrows);
// the reasons of the group's entries from Y = the previous ranks [tile][n][G]; nothing is launched without reasons()
int32_t why_group(rwr_graph *g, WhyEnd &w, int G, int tg, const int32_t *slot_k, int32_t top_n, const double *Y, hipStream_t s);
// after the last group and copy_lists_back's synchronisation: the extra tables
int32_t why_copy_back(rwr_graph *g, WhyEnd &w, int32_t K, int32_t top_n);

}  // namespace rwr
