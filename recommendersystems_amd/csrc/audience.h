// The audience of an item (internal; audience.hip): K reverse walks over the raw out-lists, ranked by the
// ranked end of the typed batch.
#pragma once
#include "engine.h"

namespace rwr {

// The driver of rwr_recommend_audience_batch: the arguments as audience_plan.h's audience_check passed them, K > 0, a nonneg
// graph, d in [0, 1].  List k ranks the rows s of cand_type (-1: of any type) by S_k[s] ~ x_T^(s)[targets[k]]; the rows with
// a raw link to targets[k] whose type has its bit in etype_mask are left out, targets[k] itself too when exclude_self.
// nodes may be nullptr.  `who` names the entry in the messages.
int32_t audience_body(rwr_graph *g, int32_t K, const int32_t *targets, double d, int32_t n_iter, int32_t cand_type,
                      uint32_t etype_mask, int32_t exclude_self, int32_t top_n, int64_t *ids, double *scores, int32_t *nodes,
                      int32_t *counts, const char *who);

}  // namespace rwr
