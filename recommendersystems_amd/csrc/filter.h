// Caller-set candidate pools and per-seed deny lists of the ranked walks (internal; filter.hip): what the
// filtered entries hand to typed.hip's driver beside the typed entries' arguments, and the call-scoped candidate list.
#pragma once
#include "filter_plan.h"
#include "iterate.h"
#include "ranked_end.h"

namespace rwr {

// the pool is one for the whole call, the deny lists are CSR over batch positions; both as filter_check passed them
struct CallFilter {
    int64_t pool_count = -1;               // < 0: no pool
    const int32_t *pool_idx = nullptr;     // host, any order, duplicates allowed
    const int64_t *deny_ptr = nullptr;     // host; nullptr: no deny lists
    const int32_t *deny_idx = nullptr;
};

// The rows that are candidates of this call (filter_plan.h), ascending, built on g->stream into `list` (the caller's: it
// must outlive the kernels that read it); *nrows = their number.  Call it on an idle stream and before the workspace is
// sized; the stream is idle on return.  Booked as prof.rank.
int32_t filter_rows_build(rwr_graph *g, int32_t cand_type, int64_t pool_count, const int32_t *pool_idx, DevBuf<int32_t> &list,
                          int32_t *nrows, Profile &prof);
// typed.hip: cand_plan.h's one-workgroup scan of nb block counts in off[0 .. nb], and the driver of the typed entries
void launch_cand_scan(int32_t nb, int32_t *off, hipStream_t s);
int32_t typed_body(rwr_graph *g, const int32_t *seeds, int32_t K, double d, int32_t n_iter, int32_t cand_type, uint32_t mask,
                   int32_t exclude_self, RankedEnd &end, const CallFilter *flt);

}  // namespace rwr
