// The host plan of the audience entries over weighted target sets (rwr_recommend_audience_set_batch,
// rwr_recommend_audience_set_positions_batch): the call as both entries describe it, the ONE ladder of argument
// checks with the status and the message of every refusal, the merge of members that repeat in a set, the (slot, row, weight)
// pairs from which a tile group's g_0 is written, and the target-to-column tables of the in-link exclusion for sets.
// rwr_recommend_audience_batch runs the same description with one-member unit sets.  Plain C++17 without HIP, so that
// tests/cpp/audience_set_plan_check.cpp checks all of it on the host.
#pragma once

#include <algorithm>
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

#include "../../include/rwr.h"
#include "audience_plan.h"
#include "eval_plan.h"
#include "exclude_plan.h"

namespace rwr {

// ---- the call ----------------------------------------------------------------------------------------------------------------
enum AudDest : int32_t {
    AUD_LISTS = 0,       // K x top_n ranked lists (out_id, out_score, out_node, out_count)
    AUD_POSITIONS = 1,   // position and score of every test id in its set's whole list, and the lists' lengths
};

struct AudCall {
    // the sets, CSR over batch positions (host): members set_idx[set_ptr[k] .. set_ptr[k + 1]), weights set_w beside them
    // (nullptr: every weight 1.0)
    int32_t K = 0;
    const int64_t *set_ptr = nullptr;
    const int32_t *set_idx = nullptr;
    const double *set_w = nullptr;
    int32_t n_iter = 0;
    int32_t cand_type = -1;                // -1: nodes of every type
    uint32_t etype_mask = 0;
    int32_t exclude_members = 0;
    // the pool (host, any order, duplicates allowed), one for the whole call; n_pool < 0: none, pool_idx is not read
    int32_t n_pool = -1;
    const int32_t *pool_idx = nullptr;
    // the deny lists, CSR over batch positions (host); deny_ptr == nullptr: none
    const int64_t *deny_ptr = nullptr;
    const int32_t *deny_idx = nullptr;
    // the destination
    AudDest dest = AUD_LISTS;
    int32_t top_n = 0;                     // AUD_LISTS
    int32_t top_n_max = AUD_TOP_N_MAX;     // ... its limit: the select path's, or the long entry's (long_plan.h)
    int64_t *out_id = nullptr;
    double *out_score = nullptr;           // AUD_LISTS: K x top_n; AUD_POSITIONS: test_ptr[K], may be nullptr
    int32_t *out_node = nullptr;           // may be nullptr
    int32_t *out_count = nullptr;
    const int64_t *test_ptr = nullptr, *test_ids = nullptr;   // AUD_POSITIONS
    int64_t *out_pos = nullptr;
    int64_t *out_len = nullptr;            // may be nullptr
};

// a weight is finite and inside [2^-256, 2^256]: with scores <= n * (sum of a set's weights) nothing overflows or leaves
// the normal range by the weights alone
constexpr double AUD_W_MIN = 0x1p-256, AUD_W_MAX = 0x1p256;
inline bool aud_weight_ok(double a) { return a >= AUD_W_MIN && a <= AUD_W_MAX; }   // (false for a NaN)

// ---- the ladder --------------------------------------------------------------------------------------------------------------
// rwr.h documents this order.  The handle's state (poisoned) belongs to the first step and the graph's and the damping
// factor's domain to the step before the no-op: the entry (api.hip) looks at both, in their places.
enum AudSetVerdict : int32_t {
    AUDSET_OK = 0,
    AUDSET_NULL_GRAPH,        // 1                                                                   (RWR_E_INVALID)
    AUDSET_NEGATIVE_K,        // 2                                                                   (RWR_E_INVALID)
    AUDSET_NULL_ARG,          // 2: K > 0 with NULL set_ptr; AUD_LISTS: NULL out_id, out_score or out_count (RWR_E_INVALID)
    AUDSET_BAD_PTR0,          // 3: set_ptr[0] != 0                                                  (RWR_E_INVALID)
    AUDSET_PTR_DECREASES,     // 3: set_ptr[bad_k + 1] < set_ptr[bad_k]                              (RWR_E_INVALID)
    AUDSET_EMPTY_SET,         // 3: set bad_k has no member                                          (RWR_E_INVALID)
    AUDSET_NULL_IDX,          // 3: NULL set_idx                                                     (RWR_E_INVALID)
    AUDSET_MEMBER_RANGE,      // 3: member bad_index at position bad_pos of set bad_k is outside [0, n) (RWR_E_RANGE)
    AUDSET_WEIGHT_RANGE,      // 3: weight bad_w at position bad_pos of set bad_k                    (RWR_E_RANGE)
    AUDSET_TOP_N_RANGE,       // 4: AUD_LISTS: top_n outside [1, top_n_max]                          (RWR_E_RANGE)
    AUDSET_NEGATIVE_ITER,     // 5: n_iter < 0                                                       (RWR_E_INVALID)
    AUDSET_BAD_CAND_TYPE,     // 5a: cand_type outside [-1, 255]                                     (RWR_E_INVALID)
    AUDSET_BAD_MASK,          // 5b: a mask bit >= AUD_EDGE_TYPES                                    (RWR_E_INVALID)
    AUDSET_NULL_POOL,         // 6: n_pool > 0 with a NULL pool_idx                                  (RWR_E_INVALID)
    AUDSET_POOL_RANGE,        // 6: pool_idx[bad_pos] = bad_index is outside [0, n)                  (RWR_E_RANGE)
    AUDSET_DENY_BAD_PTR0,     // 7: exclude_check over the deny lists, its four verdicts in its order
    AUDSET_DENY_PTR_DECREASES,
    AUDSET_DENY_NULL_IDX,
    AUDSET_DENY_BAD_INDEX,    //    (RWR_E_RANGE; the three before it RWR_E_INVALID)
    AUDSET_TEST_NULL_PTR,     // 8: AUD_POSITIONS: eval_check over the test sets and out_pos, its six verdicts in its order
    AUDSET_TEST_NULL_OUT,
    AUDSET_TEST_BAD_PTR0,
    AUDSET_TEST_PTR_DECREASES,
    AUDSET_TEST_NULL_IDS,
    AUDSET_TEST_SET_TOO_LARGE,   // (RWR_E_UNSUPPORTED; the five before it RWR_E_INVALID)
};
static_assert(EXCLUDE_BAD_INDEX - EXCLUDE_BAD_PTR0 == AUDSET_DENY_BAD_INDEX - AUDSET_DENY_BAD_PTR0 &&
                  EVAL_SET_TOO_LARGE - EVAL_NULL_PTR == AUDSET_TEST_SET_TOO_LARGE - AUDSET_TEST_NULL_PTR,
              "the deny and test verdicts are exclude_check's and eval_check's, in their order");

struct AudSetCheck {
    AudSetVerdict verdict = AUDSET_OK;
    int32_t bad_k = -1;       // the first offending batch position
    int64_t bad_pos = -1;     // MEMBER_RANGE / WEIGHT_RANGE: the position inside set bad_k; POOL_RANGE: the pool position
    int32_t bad_index = 0;    // MEMBER_RANGE, POOL_RANGE, DENY_BAD_INDEX: the index found there
    double bad_w = 0.0;       // WEIGHT_RANGE: the weight found there
};

inline AudSetCheck audience_set_check(const AudCall &a, bool have_graph, int32_t n)
{
    AudSetCheck c;
    const bool lists = a.dest == AUD_LISTS;
    const int32_t K = a.K;
    const auto is = [&c](AudSetVerdict v) { c.verdict = v; return c; };
    if (!have_graph) return is(AUDSET_NULL_GRAPH);
    if (K < 0) return is(AUDSET_NEGATIVE_K);
    if (K > 0 && (!a.set_ptr || (lists && (!a.out_id || !a.out_score || !a.out_count)))) return is(AUDSET_NULL_ARG);
    if (K > 0) {
        if (a.set_ptr[0] != 0) return is(AUDSET_BAD_PTR0);
        for (int32_t k = 0; k < K; ++k)
            if (a.set_ptr[k + 1] < a.set_ptr[k]) { c.bad_k = k; return is(AUDSET_PTR_DECREASES); }
        for (int32_t k = 0; k < K; ++k)
            if (a.set_ptr[k + 1] == a.set_ptr[k]) { c.bad_k = k; return is(AUDSET_EMPTY_SET); }
        if (!a.set_idx) return is(AUDSET_NULL_IDX);
        for (int32_t k = 0; k < K; ++k)
            for (int64_t q = a.set_ptr[k]; q < a.set_ptr[k + 1]; ++q) {
                c.bad_k = k, c.bad_pos = q - a.set_ptr[k];
                if (a.set_idx[q] < 0 || a.set_idx[q] >= n) { c.bad_index = a.set_idx[q]; return is(AUDSET_MEMBER_RANGE); }
                if (a.set_w && !aud_weight_ok(a.set_w[q])) { c.bad_w = a.set_w[q]; return is(AUDSET_WEIGHT_RANGE); }
            }
        c.bad_k = -1, c.bad_pos = -1;
    }
    if (lists && (a.top_n < 1 || a.top_n > a.top_n_max)) return is(AUDSET_TOP_N_RANGE);
    if (a.n_iter < 0) return is(AUDSET_NEGATIVE_ITER);
    if (a.cand_type < -1 || a.cand_type > 255) return is(AUDSET_BAD_CAND_TYPE);
    if (a.etype_mask >> AUD_EDGE_TYPES) return is(AUDSET_BAD_MASK);
    if (a.n_pool > 0 && !a.pool_idx) return is(AUDSET_NULL_POOL);
    for (int32_t q = 0; q < a.n_pool; ++q)
        if (a.pool_idx[q] < 0 || a.pool_idx[q] >= n) {
            c.bad_pos = q, c.bad_index = a.pool_idx[q];
            return is(AUDSET_POOL_RANGE);
        }
    if (a.deny_ptr) {
        const ExcludeCheck d = exclude_check(n, K, a.deny_ptr, a.deny_idx);
        if (d.verdict != EXCLUDE_OK) {
            c.bad_k = d.bad_k, c.bad_index = d.bad_index;
            return is((AudSetVerdict)(AUDSET_DENY_BAD_PTR0 + (d.verdict - EXCLUDE_BAD_PTR0)));
        }
    }
    if (!lists) {   // (out_pos stands where the evaluating entries have their two result arrays)
        const EvalCheck e = eval_check(K, a.test_ptr, a.test_ids, a.out_pos, a.out_pos);
        if (e.verdict != EVAL_OK) {
            c.bad_k = e.bad_k;
            return is((AudSetVerdict)(AUDSET_TEST_NULL_PTR + (e.verdict - EVAL_NULL_PTR)));
        }
    }
    return c;   // (the domain, then K == 0: api.hip)
}

// ---- a verdict as status and message -----------------------------------------------------------------------------------------
struct AudStatus {
    int32_t status = RWR_OK;
    char text[512] = "";      // (the length of the thread's error string)
};

inline AudStatus aud_refusal(int32_t status, const char *fmt, ...)
{
    AudStatus s;
    s.status = status;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(s.text, sizeof(s.text), fmt, ap);
    va_end(ap);
    return s;
}

// AUDSET_OK: RWR_OK, no text.  a and n as the check took them.
inline AudStatus audience_set_status(const char *who, const AudSetCheck &c, const AudCall &a, int32_t n)
{
    switch (c.verdict) {
        case AUDSET_OK: break;
        case AUDSET_NULL_GRAPH: return aud_refusal(RWR_E_INVALID, "%s: NULL graph", who);
        case AUDSET_NEGATIVE_K: return aud_refusal(RWR_E_INVALID, "%s: negative K", who);
        case AUDSET_NULL_ARG:
            return aud_refusal(RWR_E_INVALID, "%s: NULL %s", who, a.dest == AUD_LISTS ? "set_ptr, out_id, out_score or out_count" : "set_ptr");
        case AUDSET_BAD_PTR0: return aud_refusal(RWR_E_INVALID, "%s: set_ptr[0] = %lld, not 0", who, (long long)a.set_ptr[0]);
        case AUDSET_PTR_DECREASES: return aud_refusal(RWR_E_INVALID, "%s: set_ptr decreases at batch position %d", who, c.bad_k);
        case AUDSET_EMPTY_SET: return aud_refusal(RWR_E_INVALID, "%s: set %d is empty (a target set needs a member)", who, c.bad_k);
        case AUDSET_NULL_IDX: return aud_refusal(RWR_E_INVALID, "%s: NULL set_idx", who);
        case AUDSET_MEMBER_RANGE:
            return aud_refusal(RWR_E_RANGE, "%s: member %d (set %d, position %lld) is outside [0, %d)", who, c.bad_index, c.bad_k,
                               (long long)c.bad_pos, n);
        case AUDSET_WEIGHT_RANGE:
            return aud_refusal(RWR_E_RANGE, "%s: weight %g (set %d, position %lld) is not a finite number in [2^-256, 2^256]", who, c.bad_w,
                               c.bad_k, (long long)c.bad_pos);
        case AUDSET_TOP_N_RANGE: return aud_refusal(RWR_E_RANGE, "%s: top_n %d is outside [1, %d]", who, a.top_n, (int)a.top_n_max);
        case AUDSET_NEGATIVE_ITER:
            return aud_refusal(RWR_E_INVALID,
                               "%s: n_iter %d is negative (a fixed number of steps only: the threshold modes have no reverse counterpart)", who,
                               a.n_iter);
        case AUDSET_BAD_CAND_TYPE: return aud_refusal(RWR_E_INVALID, "%s: cand_type %d is outside [-1, 255]", who, a.cand_type);
        case AUDSET_BAD_MASK:
            return aud_refusal(RWR_E_INVALID, "%s: etype_mask 0x%x has a bit beyond the %u edge types", who, a.etype_mask, AUD_EDGE_TYPES);
        case AUDSET_NULL_POOL: return aud_refusal(RWR_E_INVALID, "%s: NULL pool_idx", who);
        case AUDSET_POOL_RANGE:
            return aud_refusal(RWR_E_RANGE, "%s: pool index %d (pool position %lld) is outside [0, %d)", who, c.bad_index, (long long)c.bad_pos, n);
        case AUDSET_DENY_BAD_PTR0: return aud_refusal(RWR_E_INVALID, "%s: deny_ptr[0] = %lld, not 0", who, (long long)a.deny_ptr[0]);
        case AUDSET_DENY_PTR_DECREASES: return aud_refusal(RWR_E_INVALID, "%s: deny_ptr decreases at batch position %d", who, c.bad_k);
        case AUDSET_DENY_NULL_IDX: return aud_refusal(RWR_E_INVALID, "%s: NULL deny_idx", who);
        case AUDSET_DENY_BAD_INDEX:
            return aud_refusal(RWR_E_RANGE, "%s: deny index %d (batch position %d) is outside [0, %d)", who, c.bad_index, c.bad_k, n);
        case AUDSET_TEST_NULL_PTR: return aud_refusal(RWR_E_INVALID, "%s: NULL test_ptr", who);
        case AUDSET_TEST_NULL_OUT: return aud_refusal(RWR_E_INVALID, "%s: NULL out_pos", who);
        case AUDSET_TEST_BAD_PTR0: return aud_refusal(RWR_E_INVALID, "%s: test_ptr[0] = %lld, not 0", who, (long long)a.test_ptr[0]);
        case AUDSET_TEST_PTR_DECREASES: return aud_refusal(RWR_E_INVALID, "%s: test_ptr decreases at batch position %d", who, c.bad_k);
        case AUDSET_TEST_NULL_IDS: return aud_refusal(RWR_E_INVALID, "%s: NULL test_ids", who);
        case AUDSET_TEST_SET_TOO_LARGE:
            return aud_refusal(RWR_E_UNSUPPORTED, "%s: test set %d holds more than INT32_MAX ids", who, c.bad_k);
    }
    return AudStatus{};
}

// ---- the merge of members that repeat in a set ---------------------------------------------------------------------------------
// Set k as the device sees it: its distinct members ascending, each with the sum of its weights, added in the order of the
// caller's list from the first occurrence's weight on (a member listed once keeps its weight's bits; set_w == nullptr counts
// 1.0 per occurrence).  This host code IS the model of those sums: the device only stores them.  O(sum of |set| log |set|).
struct AudSets {
    std::vector<int64_t> ptr;         // K + 1
    std::vector<int32_t> idx;         // distinct per set, ascending
    std::vector<double> w;            // > 0
    size_t largest = 0;               // the largest set's number of distinct members
};

inline AudSets aud_set_merge(int32_t K, const int64_t *set_ptr, const int32_t *set_idx, const double *set_w)
{
    AudSets m;
    m.ptr.assign(1, 0);
    std::vector<std::pair<int32_t, int64_t>> at;   // (member, position in the caller's list)
    for (int32_t k = 0; k < K; ++k) {
        at.clear();
        for (int64_t q = set_ptr[k]; q < set_ptr[k + 1]; ++q) at.emplace_back(set_idx[q], q);
        std::sort(at.begin(), at.end());           // (positions ascending inside a member: list order)
        const size_t first = m.idx.size();
        for (size_t j = 0; j < at.size(); ++j) {
            const double a = set_w ? set_w[at[j].second] : 1.0;
            if (j == 0 || at[j].first != at[j - 1].first) {
                m.idx.push_back(at[j].first);
                m.w.push_back(a);
            } else {
                m.w.back() = m.w.back() + a;
            }
        }
        m.largest = std::max(m.largest, m.idx.size() - first);
        m.ptr.push_back((int64_t)m.idx.size());
    }
    return m;
}

// ---- g_0: the (slot, row, weight) pairs of every tile group ----------------------------------------------------------------------
// slot_k[slot] = the batch position of the set in that slot, -1 = padding; slots_per_group slots form a tile group.  The
// pairs come out ordered by slot, a slot's in its merged set's order; those of group gi are [group_off[gi], group_off[gi + 1]),
// their slot counted from the group's first.  Cell (row, slot) occurs once: k_rev_init_sets stores, it does not add.
struct AudSetPairs {
    std::vector<int32_t> slot, row;
    std::vector<double> w;
    std::vector<int64_t> group_off;   // groups + 1
};

inline AudSetPairs aud_set_pairs(const AudSets &m, size_t nslots, const int32_t *slot_k, size_t slots_per_group)
{
    AudSetPairs p;
    const size_t ngroups = slots_per_group ? (nslots + slots_per_group - 1) / slots_per_group : 0;
    const int64_t K = (int64_t)m.ptr.size() - 1;
    p.group_off.assign(ngroups + 1, 0);
    for (size_t q = 0; q < nslots; ++q) {
        const size_t grp = q / slots_per_group;
        const int32_t k = slot_k[q];
        if (k >= 0 && k < K)
            for (int64_t j = m.ptr[(size_t)k]; j < m.ptr[(size_t)k + 1]; ++j) {
                p.slot.push_back((int32_t)(q - grp * slots_per_group));
                p.row.push_back(m.idx[(size_t)j]);
                p.w.push_back(m.w[(size_t)j]);
            }
        p.group_off[grp + 1] = (int64_t)p.slot.size();
    }
    return p;
}

// ---- the target-to-column tables of the in-link exclusion, for sets -------------------------------------------------------------
// AudTargets (audience_plan.h) as k_audience_exclude reads it: per tile group the distinct members of the group's sets
// ascending, each with the group-local slots of the sets that hold it (ascending).  A node that is a member of several sets
// of a group owns several slots; a set of several members gives one (member, slot) pair per member; a set that repeats in
// the batch sits in several slots, each with its pairs.  With one-member sets this is aud_targets() of the slots' targets.
inline AudTargets aud_set_targets(const AudSets &m, size_t nslots, const int32_t *slot_k, size_t slots_per_group)
{
    AudTargets t;
    t.group_off.push_back(0);
    t.ptr.push_back(0);
    if (slots_per_group == 0) return t;
    const int64_t K = (int64_t)m.ptr.size() - 1;
    std::vector<std::pair<int32_t, int32_t>> pairs;
    for (size_t q0 = 0; q0 < nslots; q0 += slots_per_group) {
        const size_t q1 = q0 + slots_per_group < nslots ? q0 + slots_per_group : nslots;
        pairs.clear();
        for (size_t q = q0; q < q1; ++q) {
            const int32_t k = slot_k[q];
            if (k < 0 || k >= K) continue;
            for (int64_t j = m.ptr[(size_t)k]; j < m.ptr[(size_t)k + 1]; ++j) pairs.emplace_back(m.idx[(size_t)j], (int32_t)(q - q0));
        }
        std::sort(pairs.begin(), pairs.end());
        for (size_t j = 0; j < pairs.size(); ++j) {
            if (j == 0 || pairs[j].first != pairs[j - 1].first) {
                if (j != 0) t.ptr.push_back((int32_t)t.slot.size());
                t.node.push_back(pairs[j].first);
            }
            t.slot.push_back(pairs[j].second);
        }
        if (!pairs.empty()) t.ptr.push_back((int32_t)t.slot.size());
        t.group_off.push_back((int64_t)t.node.size());
    }
    return t;
}

}  // namespace rwr
