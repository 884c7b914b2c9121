// The host-side decisions of the ranking stage: its environment values, the exact head of a batch's last step
// and the candidate capacity per seed.  Plain C++17 without HIP, so that tests/cpp/rank_plan_check.cpp checks them on the host.
#pragma once

#include <cstdint>

namespace rwr {

// The environment values (rank.hip: rank_knobs; defaults: the shipped library's): RWR_RANK_SORT (!= 0: the full sort whatever
// top_n) and RWR_SEL_FUSED (0: one decision launch per select level for few seeds too) -- both read by the experiments build
// only --, RWR_RANK_FUSED (0: never rank inside the last step, 2: whatever the size), RWR_RANK_FUSED_HEAD (> 0: the head's
// rows), RWR_RANK_FUSED_CAP (> 0: a lower candidate capacity, the tests' overflow fallback), RWR_RANK_PRUNE (0: unpruned body).
struct RankKnobs {
    int sort = 0, fused = 1, fused_cap = 0, prune = 1, sel_fused = 1;
    int64_t fused_head = 0;
};

// Ranking inside the last step: the step runs over the first H rows of tail_rows[0], the select ranks those, and the rest of
// the step keeps only the rows that reach each seed's threshold.  By default from RANK_FUSED_MIN_ITEMS ITEM rows on: below,
// the select's passes over the item block are cheaper than the second sort per seed and the synchronising copy per group
// that the split adds (C3, 62 K items: -0.4 %).  H: the power of two at or above n_items / RANK_FUSED_HEAD_DIV on the
// value-free path, whose body is pruned by the head's thresholds (the head's rows are the ones with most in-links, and past
// the first 1-2 % of the rows the bound prunes nearly all of them: tools/rank_head_study.py, DESIGN §3.3.3 "A smaller
// head"); a sixteenth of the ITEM rows on the weighted path, whose body is not pruned -- a smaller head saves nothing there.
// Returns 0 when the step is not split.  select_path: top_n is within the select's range and the sort is not forced
constexpr int32_t RANK_FUSED_MIN_ITEMS = 1 << 18;
constexpr int64_t RANK_FUSED_HEAD_DIV = 96, RANK_FUSED_HEAD_DIV_WEIGHTED = 16;
inline int32_t fused_head_rows(int32_t n_items, bool value_free, int32_t top_n, bool select_path, const RankKnobs &k)
{
    if (!k.fused || !select_path || top_n < 1 || n_items <= 0 || (k.fused != 2 && n_items < RANK_FUSED_MIN_ITEMS)) return 0;
    int64_t h = 1;
    while (h * (value_free ? RANK_FUSED_HEAD_DIV : RANK_FUSED_HEAD_DIV_WEIGHTED) < (int64_t)n_items) h <<= 1;
    if (k.fused_head > 0) h = k.fused_head;
    return (int32_t)(h < (int64_t)n_items ? h : (int64_t)n_items);
}

// Candidates a seed may append beyond its head list: the merge sorts both in one workgroup's FUSED_SORT_SLOTS entries
// (rank_fused.hip checks that they are the select's SEL_SLOTS)
constexpr int FUSED_SORT_SLOTS = 4096;
inline int fused_capacity(int32_t top_n, const RankKnobs &k)
{
    const int cap = FUSED_SORT_SLOTS - top_n;
    return (k.fused_cap > 0 && k.fused_cap < cap) ? k.fused_cap : cap;
}

}  // namespace rwr
