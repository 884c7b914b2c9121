// One seed-driven typed call, as all eight entries describe it: rwr_recommend_typed_batch,
// rwr_recommend_typed_eval_batch, rwr_recommend_typed_positions_batch, rwr_recommend_filtered_batch,
// rwr_recommend_filtered_positions_batch, rwr_recommend_capped_batch, rwr_recommend_capped_positions_batch and
// rwr_recommend_explained_batch.  An entry fills a TypedCall; typed_call_check() is the ONE ladder of argument checks --
// every entry's documented order of refusals is this ladder with the steps that do not apply to it left out -- and
// call_status() the one place that words a refusal; typed.hip's driver runs the same description.  Plain C++17 without HIP,
// so that tests/cpp/typed_call_check.cpp checks the ladder and every message on the host.
#pragma once

#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "../../include/rwr.h"
#include "eval_plan.h"
#include "exclude_plan.h"
#include "explain_plan.h"

namespace rwr {

enum CallDest : int32_t {
    CALL_LISTS = 0,      // K x top_n ranked lists (ids, scores, counts), with reasons when the entry asks for them
    CALL_EVAL = 1,       // Hits / average precision of every seed's whole list against its test set, cut to top_n when > 0
    CALL_POSITIONS = 2,  // position and score of every test id in its seed's whole list
};

struct TypedCall {
    // the walk
    const int32_t *seeds = nullptr;
    int32_t K = 0;
    int32_t cand_type = 0;                 // FILTER_ANY_TYPE: nodes of every type, where the entry allows it (any_type)
    uint32_t excl_edge_mask = 0;
    int32_t exclude_self = 0;
    // the pool (host, any order, duplicates allowed); pool_count < 0: none, pool_idx is not read
    int64_t pool_count = -1;
    const int32_t *pool_idx = nullptr;
    // the deny lists, CSR over batch positions (host); deny_ptr == nullptr: none
    const int64_t *deny_ptr = nullptr;
    const int32_t *deny_idx = nullptr;
    // the group cap: n host labels (< 0: never capped); group_of == nullptr: no cap, group_cap is not looked at
    const int32_t *group_of = nullptr;
    int32_t group_cap = 0;
    // the destination.  CALL_LISTS: top_n, ids, scores, counts -- the pointers that count as outputs in the NULL-argument
    // step; the other two have none there, their result arrays are eval_check's concern
    CallDest dest = CALL_LISTS;
    int32_t top_n = 0;
    int64_t *ids = nullptr;
    double *scores = nullptr;
    int32_t *counts = nullptr;
    // ... reasons on the lists (the explained entry): nodes and why_total may be nullptr, why_src / why_term with n_why == 0
    int32_t n_why = 0;
    int32_t *nodes = nullptr, *why_src = nullptr;
    double *why_term = nullptr;
    int64_t *why_total = nullptr;
    // CALL_EVAL and CALL_POSITIONS: the test sets, CSR over batch positions, and list_len (may be nullptr)
    const int64_t *test_ptr = nullptr, *test_ids = nullptr;
    int64_t *list_len = nullptr;
    int64_t *n_hits = nullptr;             // CALL_EVAL
    double *sum_precision = nullptr;
    int64_t *pos_out = nullptr;            // CALL_POSITIONS
    double *score_out = nullptr;
    // two facts of the entry beside the destination: is cand_type FILTER_ANY_TYPE legal (the filtered, capped and explained
    // entries), and what its top_n limit's message appends
    bool any_type = false;
    const char *top_n_hint = "";
    // the long entry (long_plan.h) replaces the ladder's top_n limit: > 0: this one instead of the select path's, worded
    // with top_n_what
    int32_t top_n_max = 0;
    const char *top_n_what = "the select path's limit";
};

enum CallVerdict : int32_t {
    CALL_OK = 0,
    CALL_NOOP,                // K == 0 with a graph: nothing to do, RWR_OK
    CALL_NULL_GRAPH,          // refused before anything else                              (RWR_E_INVALID)
    CALL_NEGATIVE_K,          //                                                           (RWR_E_INVALID)
    CALL_NULL_ARG,            // NULL seeds, or CALL_LISTS with NULL ids, scores or counts (RWR_E_INVALID)
    CALL_BAD_TOP_N,           // CALL_LISTS: top_n < 1                                     (RWR_E_INVALID)
    CALL_BAD_CAND_TYPE,       // cand_type outside [0, 255], or [-1, 255] with any_type    (RWR_E_INVALID)
    CALL_BAD_MASK,            // a mask bit >= TYPED_EDGE_TYPES                            (RWR_E_INVALID)
    CALL_SEED_RANGE,          // seeds[bad_k] = bad_seed is outside [0, n)                 (RWR_E_RANGE)
    CALL_NULL_POOL,           // pool_count > 0 with a NULL pool_idx                       (RWR_E_INVALID)
    CALL_POOL_RANGE,          // pool_idx[bad_pos] = bad_index is outside [0, n)           (RWR_E_RANGE)
    CALL_DENY_BAD_PTR0,       // exclude_check over the deny lists: deny_ptr[0] != 0       (RWR_E_INVALID)
    CALL_DENY_PTR_DECREASES,  // ... deny_ptr[bad_k + 1] < deny_ptr[bad_k]                 (RWR_E_INVALID)
    CALL_DENY_NULL_IDX,       // ... deny_idx == NULL while deny_ptr[K] > 0                (RWR_E_INVALID)
    CALL_DENY_BAD_INDEX,      // ... member bad_index of list bad_k is outside [0, n)      (RWR_E_RANGE)
    CALL_TEST_NULL_PTR,       // eval_check over the test sets: test_ptr == NULL           (RWR_E_INVALID)
    CALL_TEST_NULL_OUT,       // ... n_hits or sum_precision (CALL_EVAL), pos_out (CALL_POSITIONS) == NULL (RWR_E_INVALID)
    CALL_TEST_BAD_PTR0,       // ... test_ptr[0] != 0                                      (RWR_E_INVALID)
    CALL_TEST_PTR_DECREASES,  // ... test_ptr[bad_k + 1] < test_ptr[bad_k]                 (RWR_E_INVALID)
    CALL_TEST_NULL_IDS,       // ... test_ids == NULL while test_ptr[K] > 0                (RWR_E_INVALID)
    CALL_TEST_SET_TOO_LARGE,  // ... set bad_k holds more than EVAL_SET_MAX ids            (RWR_E_UNSUPPORTED)
    CALL_BAD_CAP,             // group_of != NULL with group_cap < 1                       (RWR_E_INVALID)
    CALL_BAD_N_WHY,           // n_why < 0                                                 (RWR_E_INVALID)
    CALL_NULL_WHY,            // n_why > 0 with a NULL why_src or why_term                 (RWR_E_INVALID)
    CALL_TOP_N_LIMIT,         // CALL_LISTS: top_n > top_n_max, the select path's limit -- or the call's own (RWR_E_UNSUPPORTED)
    CALL_CAP_LIMIT,           // group_of != NULL with group_cap > CAP_MAX                 (RWR_E_UNSUPPORTED)
    CALL_WHY_LIMIT,           // n_why > WHY_MAX                                           (RWR_E_UNSUPPORTED)
};

struct CallCheck {
    CallVerdict verdict = CALL_OK;
    int32_t bad_k = -1;       // SEED_RANGE, DENY_PTR_DECREASES / DENY_BAD_INDEX, TEST_PTR_DECREASES / TEST_SET_TOO_LARGE: the first
                              // offending batch position
    int32_t bad_seed = 0;     // SEED_RANGE: the seed found there
    int64_t bad_pos = -1;     // POOL_RANGE: the first offending position of the pool ...
    int32_t bad_index = 0;    // ... and the index found there; DENY_BAD_INDEX: the member found in list bad_k
};

inline CallVerdict call_deny_verdict(ExcludeVerdict v) { return (CallVerdict)(CALL_DENY_BAD_PTR0 + (v - EXCLUDE_BAD_PTR0)); }
inline CallVerdict call_test_verdict(EvalVerdict v) { return (CallVerdict)(CALL_TEST_NULL_PTR + (v - EVAL_NULL_PTR)); }
static_assert(EXCLUDE_BAD_INDEX - EXCLUDE_BAD_PTR0 == CALL_DENY_BAD_INDEX - CALL_DENY_BAD_PTR0 &&
                  EVAL_SET_TOO_LARGE - EVAL_NULL_PTR == CALL_TEST_SET_TOO_LARGE - CALL_TEST_NULL_PTR,
              "the deny and test verdicts are exclude_check's and eval_check's, in their order");

// The ladder.  have_graph and n: the handle and its node count (n is not read without a graph); top_n_max: the select path's
// limit.  (The graph's and the damping factor's domain come after all of it: api.hip.)
inline CallCheck typed_call_check(const TypedCall &a, bool have_graph, int32_t n, int32_t top_n_max)
{
    CallCheck c;
    const bool lists = a.dest == CALL_LISTS;
    const auto is = [&c](CallVerdict v) { c.verdict = v; return c; };
    if (!have_graph) return is(CALL_NULL_GRAPH);
    if (a.K < 0) return is(CALL_NEGATIVE_K);
    if (a.K == 0) return is(CALL_NOOP);
    if (!a.seeds || (lists && (!a.ids || !a.scores || !a.counts))) return is(CALL_NULL_ARG);
    if (lists && a.top_n < 1) return is(CALL_BAD_TOP_N);
    if (a.cand_type < (a.any_type ? FILTER_ANY_TYPE : 0) || a.cand_type > 255) return is(CALL_BAD_CAND_TYPE);
    if (a.excl_edge_mask >> TYPED_EDGE_TYPES) return is(CALL_BAD_MASK);
    for (int32_t k = 0; k < a.K; ++k)
        if (a.seeds[k] < 0 || a.seeds[k] >= n) {
            c.bad_k = k, c.bad_seed = a.seeds[k];
            return is(CALL_SEED_RANGE);
        }
    if (a.pool_count > 0 && !a.pool_idx) return is(CALL_NULL_POOL);
    for (int64_t q = 0; q < a.pool_count; ++q)
        if (a.pool_idx[q] < 0 || a.pool_idx[q] >= n) {
            c.bad_pos = q, c.bad_index = a.pool_idx[q];
            return is(CALL_POOL_RANGE);
        }
    if (a.deny_ptr) {
        const ExcludeCheck d = exclude_check(n, a.K, a.deny_ptr, a.deny_idx);
        if (d.verdict != EXCLUDE_OK) {
            c.bad_k = d.bad_k, c.bad_index = d.bad_index;
            return is(call_deny_verdict(d.verdict));
        }
    }
    if (!lists) {   // (pos_out stands where the evaluating entry has its two result arrays)
        const EvalCheck e = a.dest == CALL_EVAL ? eval_check(a.K, a.test_ptr, a.test_ids, a.n_hits, a.sum_precision)
                                                : eval_check(a.K, a.test_ptr, a.test_ids, a.pos_out, a.pos_out);
        if (e.verdict != EVAL_OK) {
            c.bad_k = e.bad_k;
            return is(call_test_verdict(e.verdict));
        }
    }
    if (a.group_of && a.group_cap < 1) return is(CALL_BAD_CAP);
    if (lists && a.n_why < 0) return is(CALL_BAD_N_WHY);
    if (lists && a.n_why > 0 && (!a.why_src || !a.why_term)) return is(CALL_NULL_WHY);
    if (lists && a.top_n > (a.top_n_max > 0 ? a.top_n_max : top_n_max)) return is(CALL_TOP_N_LIMIT);
    if (a.group_of && a.group_cap > CAP_MAX) return is(CALL_CAP_LIMIT);
    if (lists && a.n_why > WHY_MAX) return is(CALL_WHY_LIMIT);
    return c;
}

// ---- the arguments rwr_recommend_restart_typed_batch adds to rwr_recommend_restart_batch's -----------------------------------
// After the graph, K and the pointers' presence, before the vectors and the sets are looked at: top_n's lower bound, the
// candidate type, the mask, top_n's limit (the select path's, as the typed seed entry).  The positions entry has no top_n:
// it passes 1, 1.
inline CallVerdict restart_typed_check(int32_t top_n, int32_t top_n_max, int32_t cand_type, uint32_t excl_edge_mask)
{
    if (top_n < 1) return CALL_BAD_TOP_N;
    if (cand_type < 0 || cand_type > 255) return CALL_BAD_CAND_TYPE;
    if (excl_edge_mask >> TYPED_EDGE_TYPES) return CALL_BAD_MASK;
    if (top_n > top_n_max) return CALL_TOP_N_LIMIT;
    return CALL_OK;
}

// ---- a verdict as status and message ---------------------------------------------------------------------------------------
struct CallStatus {
    int32_t status = RWR_OK;
    char text[512] = "";      // (the length of the thread's error string)
};

inline CallStatus call_refusal(int32_t status, const char *fmt, ...)
{
    CallStatus s;
    s.status = status;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(s.text, sizeof(s.text), fmt, ap);
    va_end(ap);
    return s;
}

// eval_check's verdict on the test sets and result arrays of an evaluating entry; outs: the result arrays EVAL_NULL_OUT
// names for this entry
inline CallStatus eval_status(const char *who, const EvalCheck &c, const int64_t *test_ptr, const char *outs)
{
    switch (c.verdict) {
        case EVAL_OK: break;
        case EVAL_NULL_PTR: return call_refusal(RWR_E_INVALID, "%s: NULL test_ptr", who);
        case EVAL_NULL_OUT: return call_refusal(RWR_E_INVALID, "%s: NULL %s", who, outs);
        case EVAL_BAD_PTR0: return call_refusal(RWR_E_INVALID, "%s: test_ptr[0] = %lld, not 0", who, (long long)test_ptr[0]);
        case EVAL_PTR_DECREASES: return call_refusal(RWR_E_INVALID, "%s: test_ptr decreases at batch position %d", who, c.bad_k);
        case EVAL_NULL_IDS: return call_refusal(RWR_E_INVALID, "%s: NULL test_ids", who);
        case EVAL_SET_TOO_LARGE: return call_refusal(RWR_E_UNSUPPORTED, "%s: test set %d holds more than INT32_MAX ids", who, c.bad_k);
    }
    return CallStatus{};
}

// A CallCheck's verdict as status and message (CALL_OK and CALL_NOOP: RWR_OK, no text).  a: the call, for the numbers the
// texts quote and the entry's wording -- the restart-vector entries fill in what restart_typed_check looked at; n and
// top_n_max as the check took them.
inline CallStatus call_status(const char *who, const CallCheck &c, const TypedCall &a, int32_t n, int32_t top_n_max)
{
    switch (c.verdict) {
        case CALL_OK:
        case CALL_NOOP: break;
        case CALL_NULL_GRAPH: return call_refusal(RWR_E_INVALID, "%s: NULL graph", who);
        case CALL_NEGATIVE_K: return call_refusal(RWR_E_INVALID, "%s: negative K", who);
        case CALL_NULL_ARG: return call_refusal(RWR_E_INVALID, "%s: NULL %s", who, a.dest == CALL_LISTS ? "seeds, ids, scores or counts" : "seeds");
        case CALL_BAD_TOP_N: return call_refusal(RWR_E_INVALID, "%s: top_n must be >= 1", who);
        case CALL_BAD_CAND_TYPE:
            return call_refusal(RWR_E_INVALID, "%s: cand_type %d is outside [%d, 255]", who, a.cand_type, a.any_type ? FILTER_ANY_TYPE : 0);
        case CALL_BAD_MASK:
            return call_refusal(RWR_E_INVALID, "%s: excl_edge_mask 0x%x has a bit beyond the %u edge types", who, a.excl_edge_mask, TYPED_EDGE_TYPES);
        case CALL_SEED_RANGE: return call_refusal(RWR_E_RANGE, "%s: seed %d (batch position %d) is outside [0, %d)", who, c.bad_seed, c.bad_k, n);
        case CALL_NULL_POOL: return call_refusal(RWR_E_INVALID, "%s: NULL pool_idx", who);
        case CALL_POOL_RANGE:
            return call_refusal(RWR_E_RANGE, "%s: pool index %d (pool position %lld) is outside [0, %d)", who, c.bad_index, (long long)c.bad_pos, n);
        case CALL_DENY_BAD_PTR0: return call_refusal(RWR_E_INVALID, "%s: deny_ptr[0] = %lld, not 0", who, (long long)a.deny_ptr[0]);
        case CALL_DENY_PTR_DECREASES: return call_refusal(RWR_E_INVALID, "%s: deny_ptr decreases at batch position %d", who, c.bad_k);
        case CALL_DENY_NULL_IDX: return call_refusal(RWR_E_INVALID, "%s: NULL deny_idx", who);
        case CALL_DENY_BAD_INDEX:
            return call_refusal(RWR_E_RANGE, "%s: deny index %d (batch position %d) is outside [0, %d)", who, c.bad_index, c.bad_k, n);
        case CALL_TEST_NULL_PTR:
        case CALL_TEST_NULL_OUT:
        case CALL_TEST_BAD_PTR0:
        case CALL_TEST_PTR_DECREASES:
        case CALL_TEST_NULL_IDS:
        case CALL_TEST_SET_TOO_LARGE: {
            EvalCheck e;
            e.verdict = (EvalVerdict)(EVAL_NULL_PTR + (c.verdict - CALL_TEST_NULL_PTR)), e.bad_k = c.bad_k;
            return eval_status(who, e, a.test_ptr, a.dest == CALL_POSITIONS ? "pos_out" : "n_hits or sum_precision");
        }
        case CALL_BAD_CAP: return call_refusal(RWR_E_INVALID, "%s: group_cap %d is below 1", who, a.group_cap);
        case CALL_BAD_N_WHY: return call_refusal(RWR_E_INVALID, "%s: n_why %d is below 0", who, a.n_why);
        case CALL_NULL_WHY: return call_refusal(RWR_E_INVALID, "%s: NULL why_src or why_term with n_why %d", who, a.n_why);
        case CALL_TOP_N_LIMIT:
            return call_refusal(RWR_E_UNSUPPORTED, "%s: top_n %d is beyond %s of %d entries%s", who, a.top_n, a.top_n_what,
                                a.top_n_max > 0 ? a.top_n_max : top_n_max, a.top_n_hint);
        case CALL_CAP_LIMIT:
            return call_refusal(RWR_E_UNSUPPORTED, "%s: group_cap %d is beyond the limit of RWR_GROUP_CAP_MAX = %d entries per group", who,
                                a.group_cap, (int)RWR_GROUP_CAP_MAX);
        case CALL_WHY_LIMIT:
            return call_refusal(RWR_E_UNSUPPORTED, "%s: n_why %d is beyond the limit of RWR_WHY_MAX = %d reasons per entry", who, a.n_why,
                                (int)RWR_WHY_MAX);
    }
    return CallStatus{};
}

}  // namespace rwr
