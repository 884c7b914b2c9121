// The audience of an item and of a weighted target set (internal; audience.hip): K reverse walks over
// the raw out-lists, ranked by the ranked end of the typed batch.
#pragma once
#include "audience_set_plan.h"
#include "engine.h"

namespace rwr {

// The one driver of rwr_recommend_audience_batch, rwr_recommend_audience_set_batch and
// rwr_recommend_audience_set_positions_batch: `call` as audience_set_plan.h's audience_set_check passed it (the first
// entry's own ladder, audience_plan.h's, admits a subset), K > 0, a nonneg graph, d in [0, 1].  List k ranks the rows s of
// cand_type (-1: of any type; with a pool, those of them in the pool) by S_k[s] ~ sum_v a_v x_T^(s)[v] over the merged
// members (v, a_v) of set k; the rows with a raw link to any member whose type has its bit in etype_mask are left out, the
// members too when exclude_members, and the rows of deny list k.  The destination is the lists or the test ids' positions.
// `who` names the entry in the messages.
int32_t audience_body(rwr_graph *g, const AudCall &call, double d, const char *who);

}  // namespace rwr
