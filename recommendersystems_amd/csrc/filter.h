// Caller-set candidate pools of the ranked walks (internal; filter.hip): the call-scoped candidate list, and
// the compaction it shares with the handle's per-type lists (typed.hip).
#pragma once
#include "filter_plan.h"
#include "iterate.h"
#include "ranked_end.h"

namespace rwr {

// The rows that are candidates of this call (filter_plan.h), ascending, built on g->stream into `list` (the caller's: it
// must outlive the kernels that read it); *nrows = their number.  The pool is one for the whole call (host, any order,
// duplicates allowed, as typed_call_check passed it; pool_count < 0: none).  Call it on an idle stream and before the
// workspace is sized; the stream is idle on return.  Booked as prof.rank.
int32_t filter_rows_build(rwr_graph *g, int32_t cand_type, int64_t pool_count, const int32_t *pool_idx, DevBuf<int32_t> &list,
                          int32_t *nrows, Profile &prof);
// typed.hip: cand_plan.h's one-workgroup scan of nb block counts in off[0 .. nb] (in 32 bits for lists of rows, in 64 for
// node_remove.hip's chunks of links: the one scan kernel of the library), and the whole compaction of the rows that
// filter_match(type, bitmap) accepts (bitmap: device, may be nullptr) on g->stream -- count per block into off (device,
// cand_blocks(n) + 1 cells, the caller's), scan, read-back of the total (one synchronisation), allocation of `list`, ordered
// scatter.  The scatter is launched, not waited for: off, the bitmap and list must outlive it.
void launch_cand_scan(int32_t nb, int32_t *off, hipStream_t s);
void launch_cand_scan(int64_t nb, int64_t *off, hipStream_t s);
int32_t cand_compact(rwr_graph *g, int32_t type, const uint32_t *bitmap, int32_t *off, DevBuf<int32_t> &list, int32_t *nrows);

}  // namespace rwr
