// Ranked lists beyond the select's limit (internal; long_list.hip): the fourth destination of the ranked end, for
// top_n in (SEL_MAX_K, LONG_TOP_N_MAX].  After the exclusion, the deny marks and the cap: the stock levels fix a segment's
// threshold, a bin the 128 key bits could not split is cut in list order, every entry at or above the threshold is collected
// with its row, runs of LONG_RUN entries are sorted in LDS and merged between two buffers, and the first top_n go out with
// their rows -- order (score desc, id desc, row asc), total, so the lists do not depend on the collect's append order.
#pragma once
#include "iterate.h"
#include "long_plan.h"

namespace rwr {

// The long lists of one call.  The object is declared before the driver's StreamsIdle (ranked_end.h's lifetime rule).
struct LongEnd {
    int32_t *nodes = nullptr;              // the caller's K x top_n table (host), may be nullptr
    DevBuf<int32_t> d_row;                 // K x top_n rows (-1: no entry)
    DevBuf<int32_t> d_tie;                 // per segment of a pass: the bin's last list position taken (LONG_NO_TIE: all of it)
    DevBuf<uint8_t> d_alt;                 // the second entry buffer (the first lies behind the select's state: rank_group_levels)
};

// the call's row table, in its "unused" state
int32_t long_prepare(rwr_graph *g, LongEnd &l, int32_t K, int32_t top_n, hipStream_t s);
// the ranking of a tile group over `rows` (nrows > 0, ascending), as many tiles per pass as long_tiles_per_pass allows
int32_t long_rank_group(rwr_graph *g, LongEnd &l, int G, int tg, const int32_t *slot_k, int32_t top_n, const double *X, hipStream_t s,
                        const int32_t *rows, int32_t nrows);
// after the last group and copy_lists_back's synchronisation: the rows
int32_t long_copy_back(rwr_graph *g, LongEnd &l, int32_t K, int32_t top_n);

}  // namespace rwr
