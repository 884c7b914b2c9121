// Host check of recommendersystems_amd/csrc/rank_plan.h (tests/test_rank_plan.py): the defaults of the ranking's environment
// values, the head of a batch's last step and the candidate capacity per seed, at the values the rules give at their edges.
#include "rank_plan.h"

#include <cstdio>
#include <initializer_list>

using namespace rwr;

static int failures = 0;
#define CHECK_EQ(got, want) do { const long long g_ = (got), w_ = (want); if (g_ != w_) { ++failures; \
    std::printf("FAIL %s:%d: %s = %lld, expected %lld\n", __FILE__, __LINE__, #got, g_, w_); } } while (0)

static RankKnobs knobs(int fused, int64_t head = 0, int cap = 0)
{
    RankKnobs k;
    k.fused = fused, k.fused_head = head, k.fused_cap = cap;
    return k;
}

int main()
{
    const RankKnobs def;
    CHECK_EQ(def.sort, 0);
    CHECK_EQ(def.fused, 1);
    CHECK_EQ(def.fused_head, 0);
    CHECK_EQ(def.fused_cap, 0);
    CHECK_EQ(def.prune, 1);
    CHECK_EQ(def.sel_fused, 1);
    const int32_t big = 1 << 18, top_n = 100;
    // the size threshold, and the head's share of the ITEM rows on the value-free and on the weighted path
    CHECK_EQ(fused_head_rows(big, true, top_n, true, def), 4096);
    CHECK_EQ(fused_head_rows(big, false, top_n, true, def), 16384);
    CHECK_EQ(fused_head_rows(big - 1, true, top_n, true, def), 0);
    CHECK_EQ(fused_head_rows(big - 1, false, top_n, true, def), 0);
    CHECK_EQ(fused_head_rows(big - 1, true, top_n, true, knobs(2)), 4096);
    // off: the knob, the sort path, no top_n, no items
    for (int32_t n : {1, 5, 10025, big - 1, big, 1 << 24, INT32_MAX}) CHECK_EQ(fused_head_rows(n, true, top_n, true, knobs(0)), 0);
    CHECK_EQ(fused_head_rows(big, true, top_n, false, def), 0);
    CHECK_EQ(fused_head_rows(big, true, top_n, false, knobs(2)), 0);
    CHECK_EQ(fused_head_rows(big, true, 0, true, def), 0);
    CHECK_EQ(fused_head_rows(0, true, top_n, true, def), 0);
    CHECK_EQ(fused_head_rows(0, true, top_n, true, knobs(2)), 0);
    // a head set by hand, cut to the ITEM rows
    CHECK_EQ(fused_head_rows(10025, true, top_n, true, knobs(2, 13)), 13);
    CHECK_EQ(fused_head_rows(5, true, top_n, true, knobs(2, 13)), 5);
    CHECK_EQ(fused_head_rows(big, true, top_n, true, knobs(1, 13)), 13);
    CHECK_EQ(fused_head_rows(big, false, top_n, true, knobs(1, (int64_t)1 << 40)), big);
    // the power of two at or above n_items / 96 (value-free) and n_items / 16 (weighted)
    for (int k = 0; k <= 24; ++k) {
        const int64_t n = 96ll << k;
        if (n + 1 > INT32_MAX) break;
        CHECK_EQ(fused_head_rows((int32_t)n, true, top_n, true, knobs(2)), 1ll << k);
        CHECK_EQ(fused_head_rows((int32_t)n + 1, true, top_n, true, knobs(2)), 1ll << (k + 1));
        CHECK_EQ(fused_head_rows((int32_t)(16ll << k), false, top_n, true, knobs(2)), 1ll << k);
        CHECK_EQ(fused_head_rows((int32_t)(16ll << k) + 1, false, top_n, true, knobs(2)), 1ll << (k + 1));
    }
    CHECK_EQ(fused_head_rows(1, true, top_n, true, knobs(2)), 1);
    CHECK_EQ(fused_head_rows(INT32_MAX, true, top_n, true, def), 1 << 25);   // (2^31 - 1) / 96 = 22.4 M
    // the candidate capacity: what the merge's slots leave beside the head's list, or the lower value set by hand
    CHECK_EQ(fused_capacity(5, def), 4091);
    CHECK_EQ(fused_capacity(5, knobs(1, 0, 8)), 8);
    CHECK_EQ(fused_capacity(1024, def), 3072);
    CHECK_EQ(fused_capacity(1024, knobs(1, 0, 5000)), 3072);
    CHECK_EQ(fused_capacity(1024, knobs(1, 0, 3072)), 3072);
    CHECK_EQ(fused_capacity(1024, knobs(1, 0, 3071)), 3071);
    CHECK_EQ(fused_capacity(1, knobs(1, 0, -3)), 4095);
    std::printf("%d failures\n", failures);
    return failures != 0;
}
