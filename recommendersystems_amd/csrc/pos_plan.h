// What the positions destination of a ranked end (rwr_recommend_typed_positions_batch, rwr_recommend_restart_typed_positions_batch,
// DESIGN §3.19) decides on the host on top of eval_plan()'s sets: where the answer of every caller entry lies in the device
// result arrays, and how large those are.  Carried out by eval_pos.hip.  Plain C++17 without HIP, so that
// tests/cpp/pos_plan_check.cpp checks it against a direct restatement.
//
// eval_plan() lays test set k out sorted and without duplicates at the slot that holds batch position k (slot order).  The
// device writes one position and one score per laid-out id -- arrays parallel to EvalPlan::ids, initialised to -1 / +0.0 --
// and one list length per batch position.  The caller's entries keep their order and their duplicates: entry j of set k is
// answered by the laid-out id equal to test_ids[j] in k's slot, entry_u[j] being its index into EvalPlan::ids.  Two entries
// with one id share their u; two batch positions with one seed sit in two slots and have two sets.  A batch position that no
// slot holds has nothing laid out: its entries get -1 (no answer), which pos_scatter() turns into -1 / +0.0.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "eval_plan.h"

namespace rwr {

struct PosPlan {
    std::vector<int64_t> entry_u;     // [test_ptr[K]] index into EvalPlan::ids of the caller's entry, -1 = none
    std::vector<int64_t> slot_of_k;   // [K] the (first) slot that holds batch position k, -1 = none
    // device result array sizes (elements): positions and scores (one per laid-out id), list lengths (one per batch position)
    size_t n_pos = 0, n_score = 0, n_len = 0;
};

// ev: eval_plan()'s result for the same slot assignment and sets (its verdict EVAL_OK; anything else plans nothing)
inline PosPlan pos_plan(const EvalPlan &ev, size_t nslots, const int32_t *slot_k, int32_t K, const int64_t *test_ptr,
                        const int64_t *test_ids)
{
    PosPlan p;
    if (ev.check.verdict != EVAL_OK || K <= 0) return p;
    p.n_pos = p.n_score = ev.n_ids;
    p.n_len = (size_t)K;
    p.slot_of_k.assign((size_t)K, -1);
    for (size_t slot = 0; slot < nslots; ++slot) {
        const int32_t k = slot_k[slot];
        if (k >= 0 && k < K && p.slot_of_k[(size_t)k] < 0) p.slot_of_k[(size_t)k] = (int64_t)slot;
    }
    p.entry_u.assign((size_t)test_ptr[K], -1);
    for (int32_t k = 0; k < K; ++k) {
        const int64_t slot = p.slot_of_k[(size_t)k];
        if (slot < 0) continue;
        const int64_t *lo = ev.ids.data() + ev.slot_off[(size_t)slot], *hi = ev.ids.data() + ev.slot_off[(size_t)slot + 1];
        for (int64_t j = test_ptr[k]; j < test_ptr[k + 1]; ++j) {
            const int64_t *at = std::lower_bound(lo, hi, test_ids[j]);
            if (at != hi && *at == test_ids[j]) p.entry_u[(size_t)j] = at - ev.ids.data();
        }
    }
    return p;
}

// The device arrays, copied back once, into the caller's: entry j receives the answer of its laid-out id, batch position k its
// list length.  score_out and list_len may be NULL.
inline void pos_scatter(const PosPlan &p, int32_t K, const int64_t *dev_pos, const double *dev_score, const int64_t *dev_len,
                        int64_t *pos_out, double *score_out, int64_t *list_len)
{
    for (size_t j = 0; j < p.entry_u.size(); ++j) {
        const int64_t u = p.entry_u[j];
        pos_out[j] = u < 0 ? -1 : dev_pos[u];
        if (score_out) score_out[j] = u < 0 || dev_pos[u] < 0 ? 0.0 : dev_score[u];
    }
    if (list_len)
        for (int32_t k = 0; k < K; ++k) list_len[k] = dev_len[k];
}

}  // namespace rwr
