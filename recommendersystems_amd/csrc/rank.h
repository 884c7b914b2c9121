// The ranking stage (internal): rank.hip (exclusion, sort path, small path, radix select, dangling seeds) and rank_fused.hip
// (the ranking inside a batch's last step).
#pragma once
#include "engine.h"
#include "rank_plan.h"

namespace rwr {

struct SplitLast;   // iterate.h
struct Profile;

const RankKnobs &rank_knobs();   // the ranking's environment values, read once per process
int rank_select_max_k();         // the largest top_n of the select path (SEL_MAX_K)
// the exclusion (k_exclude: X[tile][n][G], one seed per slot, -1 = none)
void launch_exclude(rwr_graph *g, int G, int tg, double *X, const int32_t *d_seeds, hipStream_t s);
// the zeroed result tables of a call: K rows of top_n entries, indexed by the caller's batch position
int32_t ensure_out_tables(rwr_graph *g, int32_t K, int32_t top_n, hipStream_t s);
// one tile by the full sort (any top_n); a tile group by the radix select (top_n <= SEL_MAX_K) over `rows` (nullptr: the ITEM rows)
int32_t rank_tile(rwr_graph *g, int G, const int32_t *d_slot_k_tile, int32_t top_n, const double *X,
                  const int32_t *d_seeds_tile, hipStream_t s);
int32_t rank_group_select(rwr_graph *g, int G, int tg, const int32_t *d_slot_k, int32_t top_n, const double *X,
                          const int32_t *d_seeds, hipStream_t s, const int32_t *rows = nullptr, int32_t nrows = 0);
// ... the select's levels alone (explain.hip follows them with a row-carrying collect and sort-and-emit): the thresholds of the
// tg * G segments in *st_out, room for SEL_SLOTS candidates of cand_size bytes per segment in *cand_out; m > 0 rows.  slots > 0
// (long_list.hip): room for `slots` candidates per segment, for a top_n beyond SEL_MAX_K
struct SelState;   // rank_keys.h
int32_t rank_group_levels(rwr_graph *g, int G, int tg, int32_t top_n, const double *X, const int32_t *d_seeds, hipStream_t s,
                          const int32_t *rows, int32_t m, size_t cand_size, SelState **st_out, void **cand_out, size_t slots = 0);
// a tile group whose exclusion has been applied: the select when top_n allows it and RWR_RANK_SORT does not force the sort
int32_t rank_group(rwr_graph *g, int G, int tg, const int32_t *d_slot_k, const int32_t *d_seeds, int32_t top_n, const double *X,
                   hipStream_t s);
// ... whose last step ran over the head only (split.taken): head select, thresholds, pruned selecting launch, merge.  *ranked =
// false: a seed's candidates overflowed -- the step has been redone whole and the exclusion applied again, rank_group is due.
// Owns the rank_fused_groups / rank_fused_fallbacks / rank_pruned_rows counters
int32_t rank_group_fused(rwr_graph *g, int G, int tg, const int32_t *d_slot_k, const int32_t *d_seeds, int32_t top_n, double *Xf,
                         SplitLast &split, Profile &prof, hipStream_t s, bool *ranked);
// the lists of dangling seeds, known without iterating (k_emit_dangling)
int32_t emit_dangling(rwr_graph *g, const std::vector<int32_t> &rows, const std::vector<int32_t> &seeds, int32_t top_n,
                      hipStream_t s);

}  // namespace rwr
