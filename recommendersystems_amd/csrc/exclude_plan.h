// Which raw links one rwr_recommend_restart_batch call looks at to mark its non-candidates, decided by
// exclude_plan() from the handle's host row pointers, the batch's slot assignment and the K exclusion sets alone and carried out
// by k_exclude_typed (ranked_end.hip).  Plain C++17 without HIP, so that tests/cpp/exclude_plan_check.cpp checks it against a
// direct walk over the members' raw lists on the host.
//
// Set k is the node list set_idx[set_ptr[k] .. set_ptr[k + 1]): the RAW out-links of type LIKE of every member are not
// candidates of vector k (Recommender.cs:20-24 applied to each member).  Vector k sits in one slot of the rank matrices; the
// slots are walked in order, slots_per_group at a time (a tile group), and a member's raw list [rowptr[i], rowptr[i + 1]) is cut
// into segments of at most EXCLUDE_SEG_MAX links -- one wave each, so that a hub user's list does not serialise on one wave.
// The segments come out ordered by slot; those of tile group gi are [group_off[gi], group_off[gi + 1]), their slot counted
// from the group's first.  A member listed twice gives its segments twice (the stores are idempotent), a member without raw
// links and an empty set give none, a padding slot (slot_k < 0) has no set.  O(sum of set sizes + segments).
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace rwr {

constexpr int64_t EXCLUDE_SEG_MAX = 4096;

enum ExcludeVerdict : int32_t {
    EXCLUDE_OK = 0,
    EXCLUDE_BAD_PTR0 = 1,      // set_ptr[0] != 0
    EXCLUDE_PTR_DECREASES = 2, // set_ptr[bad_k + 1] < set_ptr[bad_k]
    EXCLUDE_NULL_IDX = 3,      // set_idx == NULL while set_ptr[K] > 0
    EXCLUDE_BAD_INDEX = 4,     // member bad_index of set bad_k is outside [0, n)
};

struct ExcludeCheck {
    ExcludeVerdict verdict = EXCLUDE_OK;
    int32_t bad_k = -1;        // the first offending set (PTR_DECREASES / BAD_INDEX)
    int32_t bad_index = 0;     // the member found there (BAD_INDEX)
};

struct ExcludePlan {
    ExcludeCheck check;
    std::vector<int32_t> seg_slot;    // [segments] slot within its tile group
    std::vector<int64_t> seg_p0;      // [segments] raw links [p0, p1), p1 - p0 in [1, EXCLUDE_SEG_MAX]
    std::vector<int64_t> seg_p1;
    std::vector<int64_t> group_off;   // [groups + 1]
};

// The verdict on K exclusion sets over n nodes, every entry looked at before anything is planned: the pointer array first
// (start, then the first decrease), then the index array's presence, then the first member out of range.
inline ExcludeCheck exclude_check(int32_t n, int32_t K, const int64_t *set_ptr, const int32_t *set_idx)
{
    ExcludeCheck c;
    if (K <= 0) return c;
    if (set_ptr[0] != 0) { c.verdict = EXCLUDE_BAD_PTR0; return c; }
    for (int32_t k = 0; k < K; ++k)
        if (set_ptr[k + 1] < set_ptr[k]) { c.verdict = EXCLUDE_PTR_DECREASES; c.bad_k = k; return c; }
    if (set_ptr[K] > 0 && !set_idx) { c.verdict = EXCLUDE_NULL_IDX; return c; }
    for (int32_t k = 0; k < K; ++k)
        for (int64_t q = set_ptr[k]; q < set_ptr[k + 1]; ++q)
            if (set_idx[q] < 0 || set_idx[q] >= n) {
                c.verdict = EXCLUDE_BAD_INDEX; c.bad_k = k; c.bad_index = set_idx[q];
                return c;
            }
    return c;
}

// rowptr: the n + 1 row pointers of the resident raw lists.  slot_k[slot] = batch position of the vector in that slot, -1 = a
// padding slot; the nslots slots form ceil(nslots / slots_per_group) tile groups.
inline ExcludePlan exclude_plan(int32_t n, const int64_t *rowptr, size_t nslots, const int32_t *slot_k, size_t slots_per_group,
                                int32_t K, const int64_t *set_ptr, const int32_t *set_idx)
{
    ExcludePlan p;
    p.check = exclude_check(n, K, set_ptr, set_idx);
    const size_t ngroups = slots_per_group ? (nslots + slots_per_group - 1) / slots_per_group : 0;
    p.group_off.assign(ngroups + 1, 0);
    if (p.check.verdict != EXCLUDE_OK) return p;
    for (size_t slot = 0; slot < nslots; ++slot) {
        const size_t grp = slot / slots_per_group;
        const int32_t k = slot_k[slot];
        if (k >= 0 && k < K)
            for (int64_t q = set_ptr[k]; q < set_ptr[k + 1]; ++q) {
                const int64_t e = rowptr[(size_t)set_idx[q] + 1];
                for (int64_t b = rowptr[(size_t)set_idx[q]]; b < e; b += EXCLUDE_SEG_MAX) {
                    p.seg_slot.push_back((int32_t)(slot - grp * slots_per_group));
                    p.seg_p0.push_back(b);
                    p.seg_p1.push_back(e - b < EXCLUDE_SEG_MAX ? e : b + EXCLUDE_SEG_MAX);
                }
            }
        p.group_off[grp + 1] = (int64_t)p.seg_slot.size();
    }
    return p;
}

}  // namespace rwr
