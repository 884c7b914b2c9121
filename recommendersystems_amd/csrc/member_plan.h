// What the two typed ends of DESIGN §3.17 decide on the host beside the plans they share with their neighbours: the
// (slot, member) pairs whose own rows rwr_recommend_restart_typed_batch marks when exclude_members is set.  (The verdicts on
// the arguments that rwr_recommend_typed_eval_batch and rwr_recommend_restart_typed_batch add are typed_call.h's.)  Plain
// C++17 without HIP, so that tests/cpp/member_plan_check.cpp checks the pairs against brute-force loops on the host.
//
// Exclusion set k is the node list set_idx[set_ptr[k] .. set_ptr[k + 1]) (exclude_plan.h: the same sets, the same slot walk).
// A group is not recommended its own members: every member's row of its vector's column is a non-candidate.  The pairs come
// out ordered by slot, the members of a slot in the order of its set; those of tile group gi are
// [group_off[gi], group_off[gi + 1]), their slot counted from the group's first.  A member listed twice gives its pair twice
// (k_exclude_members' stores are idempotent), an empty set gives none, a padding slot (slot_k < 0) has no set.  Unlike a
// segment, a pair needs no raw link: a dangling member is marked as well.  O(sum of set sizes).
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "exclude_plan.h"

namespace rwr {

struct MemberPlan {
    ExcludeCheck check;               // exclude_check's verdict on the sets: anything but EXCLUDE_OK plans nothing
    std::vector<int32_t> pair_slot;   // [pairs] slot within its tile group
    std::vector<int32_t> pair_row;    // [pairs] the member's row, in [0, n)
    std::vector<int64_t> group_off;   // [groups + 1]
};

// slot_k[slot] = batch position of the vector in that slot, -1 = a padding slot; the nslots slots form
// ceil(nslots / slots_per_group) tile groups.
inline MemberPlan member_plan(int32_t n, size_t nslots, const int32_t *slot_k, size_t slots_per_group, int32_t K,
                              const int64_t *set_ptr, const int32_t *set_idx)
{
    MemberPlan p;
    p.check = exclude_check(n, K, set_ptr, set_idx);
    const size_t ngroups = slots_per_group ? (nslots + slots_per_group - 1) / slots_per_group : 0;
    p.group_off.assign(ngroups + 1, 0);
    if (p.check.verdict != EXCLUDE_OK) return p;
    for (size_t slot = 0; slot < nslots; ++slot) {
        const size_t grp = slot / slots_per_group;
        const int32_t k = slot_k[slot];
        if (k >= 0 && k < K)
            for (int64_t q = set_ptr[k]; q < set_ptr[k + 1]; ++q) {
                p.pair_slot.push_back((int32_t)(slot - grp * slots_per_group));
                p.pair_row.push_back(set_idx[q]);
            }
        p.group_off[grp + 1] = (int64_t)p.pair_slot.size();
    }
    return p;
}

}  // namespace rwr
