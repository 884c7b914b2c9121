// What one rwr_recommend_restart_eval_batch call puts on the device to evaluate its walks, decided on the host
// from the K test sets, the batch's slot assignment and -- per tile group -- the slots' hit counts alone; carried out by
// eval_count.hip.  Plain C++17 without HIP, so that tests/cpp/eval_plan_check.cpp checks it against a direct restatement.
//
// Test set k is test_ids[test_ptr[k] .. test_ptr[k + 1]) with HashSet<long> semantics (Experiment.cs:124): eval_plan() lays the
// sets out sorted ascending and without duplicates, in slot order -- slot_off[slot] .. slot_off[slot + 1], a padding slot
// (slot_k < 0) being empty -- so that the sets of a tile, and of a tile group (slots_per_group slots, group_off), are one
// contiguous range that a kernel addresses relative to its first slot.  Ids that no node carries stay: they hit nothing.
//
// A tile group's hits are known only after the counting launch: eval_group_layout() turns the slots' hit counts into the exact
// offsets of the hit lists, the interval counters (one more than hits per slot), the slots whose list is too long for the
// one-workgroup sort, and per tile whether its lists and counters fit the workgroup's LDS budget.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace rwr {

constexpr int64_t EVAL_SET_MAX = 0x7FFFFFFF;   // ids per test set (INT32_MAX)
constexpr int32_t EVAL_SORT_SLOTS = 4096;      // longest hit list of the one-workgroup sort (SEL_SLOTS, rank_keys.h)
// LDS a counting workgroup may take for a tile's sorted hit keys (16 B) and interval counters (4 B): 64 KiB of the CU's
// 160 KiB, so that two workgroups stay resident per CU
constexpr size_t EVAL_LDS_BYTES = 64 * 1024;

enum EvalVerdict : int32_t {
    EVAL_OK = 0,
    EVAL_NULL_PTR = 1,        // test_ptr == NULL
    EVAL_NULL_OUT = 2,        // n_hits or sum_precision == NULL
    EVAL_BAD_PTR0 = 3,        // test_ptr[0] != 0
    EVAL_PTR_DECREASES = 4,   // test_ptr[bad_k + 1] < test_ptr[bad_k]
    EVAL_NULL_IDS = 5,        // test_ids == NULL while test_ptr[K] > 0
    EVAL_SET_TOO_LARGE = 6,   // set bad_k holds more than EVAL_SET_MAX ids
};

struct EvalCheck {
    EvalVerdict verdict = EVAL_OK;
    int32_t bad_k = -1;       // the first offending set (PTR_DECREASES / SET_TOO_LARGE)
};

struct EvalPlan {
    EvalCheck check;
    std::vector<int64_t> ids;         // the sets, sorted and de-duplicated, in slot order
    std::vector<int64_t> slot_off;    // [slots + 1] into ids
    std::vector<int64_t> group_off;   // [groups + 1] into ids: group gi's sets are ids[group_off[gi] .. group_off[gi + 1])
    // device buffer sizes (elements): the sets, their offsets, the K result records; the hit counts of one tile group
    size_t n_ids = 0, n_off = 0, n_out = 0, n_group_slots = 0;
};

// The verdict on K test sets and the result arrays, every pointer entry looked at before anything is planned: the pointers'
// presence first, then the pointer array (start, then the first decrease), then the id array's presence, then the first set
// that is too large.
inline EvalCheck eval_check(int32_t K, const int64_t *test_ptr, const int64_t *test_ids, const void *n_hits,
                            const void *sum_precision)
{
    EvalCheck c;
    if (K <= 0) return c;
    if (!test_ptr) { c.verdict = EVAL_NULL_PTR; return c; }
    if (!n_hits || !sum_precision) { c.verdict = EVAL_NULL_OUT; return c; }
    if (test_ptr[0] != 0) { c.verdict = EVAL_BAD_PTR0; return c; }
    for (int32_t k = 0; k < K; ++k)
        if (test_ptr[k + 1] < test_ptr[k]) { c.verdict = EVAL_PTR_DECREASES; c.bad_k = k; return c; }
    if (test_ptr[K] > 0 && !test_ids) { c.verdict = EVAL_NULL_IDS; return c; }
    for (int32_t k = 0; k < K; ++k)
        if (test_ptr[k + 1] - test_ptr[k] > EVAL_SET_MAX) { c.verdict = EVAL_SET_TOO_LARGE; c.bad_k = k; return c; }
    return c;
}

// slot_k[slot] = batch position of the vector in that slot, -1 = a padding slot; the nslots slots form
// ceil(nslots / slots_per_group) tile groups.  The result arrays are the entry point's concern: only their presence is checked.
inline EvalPlan eval_plan(size_t nslots, const int32_t *slot_k, size_t slots_per_group, int32_t K, const int64_t *test_ptr,
                          const int64_t *test_ids, const void *n_hits, const void *sum_precision)
{
    EvalPlan p;
    p.check = eval_check(K, test_ptr, test_ids, n_hits, sum_precision);
    const size_t ngroups = slots_per_group ? (nslots + slots_per_group - 1) / slots_per_group : 0;
    p.slot_off.assign(nslots + 1, 0);
    p.group_off.assign(ngroups + 1, 0);
    p.n_off = nslots + 1;
    p.n_out = K > 0 ? (size_t)K : 0;
    p.n_group_slots = std::min(slots_per_group, nslots);
    if (p.check.verdict != EVAL_OK) return p;
    for (size_t slot = 0; slot < nslots; ++slot) {
        const int32_t k = slot_k[slot];
        if (k >= 0 && k < K && test_ptr[k + 1] > test_ptr[k]) {
            const size_t at = p.ids.size();
            p.ids.insert(p.ids.end(), test_ids + test_ptr[k], test_ids + test_ptr[k + 1]);
            std::sort(p.ids.begin() + (ptrdiff_t)at, p.ids.end());
            p.ids.erase(std::unique(p.ids.begin() + (ptrdiff_t)at, p.ids.end()), p.ids.end());
        }
        p.slot_off[slot + 1] = (int64_t)p.ids.size();
        p.group_off[slot / slots_per_group + 1] = (int64_t)p.ids.size();
    }
    p.n_ids = p.ids.size();
    return p;
}

// One tile group after its counting launch: hit_cnt[slot] hits in each of its nslots slots (tiles of G slots).
struct EvalGroupLayout {
    std::vector<int64_t> hit_off;     // [nslots + 1]: slot's hit keys are [hit_off[slot], hit_off[slot + 1]) of the group's lists;
                                      // its hit_cnt + 1 interval counters start at hit_off[slot] + slot
    std::vector<int32_t> long_slots;  // slots with more than EVAL_SORT_SLOTS hits: the radix sort
    std::vector<uint8_t> tile_lds;    // [tiles]: the tile's keys and counters fit lds_bytes
    int64_t n_hits = 0, n_counters = 0, max_long = 0;
    bool bad = false;                 // a negative count: nothing is laid out
};

inline EvalGroupLayout eval_group_layout(const int32_t *hit_cnt, size_t nslots, int G, size_t lds_bytes = EVAL_LDS_BYTES)
{
    EvalGroupLayout L;
    L.hit_off.assign(nslots + 1, 0);
    for (size_t s = 0; s < nslots; ++s) {
        if (hit_cnt[s] < 0) { L.bad = true; return L; }
        L.hit_off[s + 1] = L.hit_off[s] + hit_cnt[s];
        if (hit_cnt[s] > EVAL_SORT_SLOTS) {
            L.long_slots.push_back((int32_t)s);
            L.max_long = std::max<int64_t>(L.max_long, hit_cnt[s]);
        }
    }
    L.n_hits = L.hit_off[nslots];
    L.n_counters = L.n_hits + (int64_t)nslots;
    const size_t g = G > 0 ? (size_t)G : 1, tiles = (nslots + g - 1) / g;
    L.tile_lds.assign(tiles, 0);
    for (size_t t = 0; t < tiles; ++t) {
        const size_t s0 = t * g, s1 = std::min(nslots, s0 + g);
        const uint64_t h = (uint64_t)(L.hit_off[s1] - L.hit_off[s0]);
        L.tile_lds[t] = h * 16 + (h + (s1 - s0)) * 4 <= (uint64_t)lds_bytes;
    }
    return L;
}

}  // namespace rwr
