// The host plan of the audience entry (rwr_recommend_audience_batch): the ladder of argument checks, the
// long-row split of the reverse step, the target-to-column table of the in-link exclusion, the workspace sizes, and the
// restart-mass recurrence -- the one function audience.hip's k_rev_rho compiles too.  Plain C++17 without HIP, so that
// tests/cpp/audience_plan_check.cpp checks all of it on the host.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#if defined(__HIPCC__)
#define RWR_AUD_HD __host__ __device__
#else
#define RWR_AUD_HD
#endif

namespace rwr {

// ---- the ladder ------------------------------------------------------------------------------------------------------------
// rwr.h documents this order.  The handle's state (poisoned) belongs to the first step and the graph's and the damping
// factor's domain to the step before the no-op: the entry (api.hip) looks at both, in their places.
constexpr int32_t AUD_TOP_N_MAX = 1024;          // the select path's limit (rank_plan.h: SEL_MAX_K), as rwr_recommend_typed_batch
constexpr uint32_t AUD_EDGE_TYPES = 8;           // the mask's width in edge types (cand_plan.h: TYPED_EDGE_TYPES)

enum AudVerdict : int32_t {
    AUD_OK = 0,
    AUD_NOOP,            // K == 0 after every other check: nothing to do, RWR_OK
    AUD_NULL_GRAPH,      // 1                                                          (RWR_E_INVALID)
    AUD_NEGATIVE_K,      // 2                                                          (RWR_E_INVALID)
    AUD_NULL_ARG,        // 2: K > 0 with NULL targets, out_id, out_score or out_count (RWR_E_INVALID)
    AUD_TARGET_RANGE,    // 3: targets[bad_k] = bad_target is outside [0, n)           (RWR_E_RANGE)
    AUD_TOP_N_RANGE,     // 4: top_n outside [1, AUD_TOP_N_MAX]                        (RWR_E_RANGE)
    AUD_NEGATIVE_ITER,   // 5: n_iter < 0                                              (RWR_E_INVALID)
    AUD_BAD_CAND_TYPE,   // 5a: cand_type outside [-1, 255]                            (RWR_E_INVALID)
    AUD_BAD_MASK,        // 5b: a mask bit >= AUD_EDGE_TYPES                           (RWR_E_INVALID)
};

struct AudCheck {
    AudVerdict verdict = AUD_OK;
    int32_t bad_k = -1, bad_target = 0;
};

inline AudCheck audience_check(bool have_graph, int32_t n, int32_t K, const int32_t *targets, int32_t n_iter, int32_t cand_type,
                               uint32_t etype_mask, int32_t top_n, const void *out_id, const void *out_score, const void *out_count)
{
    AudCheck c;
    const auto is = [&c](AudVerdict v) { c.verdict = v; return c; };
    if (!have_graph) return is(AUD_NULL_GRAPH);
    if (K < 0) return is(AUD_NEGATIVE_K);
    if (K > 0 && (!targets || !out_id || !out_score || !out_count)) return is(AUD_NULL_ARG);
    for (int32_t k = 0; k < K; ++k)
        if (targets[k] < 0 || targets[k] >= n) {
            c.bad_k = k, c.bad_target = targets[k];
            return is(AUD_TARGET_RANGE);
        }
    if (top_n < 1 || top_n > AUD_TOP_N_MAX) return is(AUD_TOP_N_RANGE);
    if (n_iter < 0) return is(AUD_NEGATIVE_ITER);
    if (cand_type < -1 || cand_type > 255) return is(AUD_BAD_CAND_TYPE);
    if (etype_mask >> AUD_EDGE_TYPES) return is(AUD_BAD_MASK);
    return c;   // (the domain, then K == 0: api.hip)
}

// ---- the long-row split of the reverse step ----------------------------------------------------------------------------------
// A lane group of k_rev_spmm walks one row's out-list in list order.  Its budget is AUD_SPLIT links: the step's main launch
// sums the first AUD_SPLIT links of every row; a longer row's further links are cut into pieces of AUD_SPLIT, each summed in
// list order by a lane group of its own (k_rev_pieces) into a partial, and k_rev_join adds the partials to the first
// piece's sum in piece order -- a fixed association that depends on the row's length alone, not on the batch.
constexpr int32_t AUD_SPLIT = 512;
constexpr int32_t AUD_SHORT = 4;                 // rows of at most this many links take k_rev_spmm's loop-free path

RWR_AUD_HD inline int64_t aud_first_piece_end(int64_t p0, int64_t p1) { return p1 - p0 > AUD_SPLIT ? p0 + AUD_SPLIT : p1; }
inline int64_t aud_extra_pieces(int64_t deg) { return deg > AUD_SPLIT ? (deg - 1) / AUD_SPLIT : 0; }

struct AudLongRows {
    std::vector<int32_t> row;         // the rows of more than AUD_SPLIT links, ascending
    std::vector<int32_t> first;       // rows + 1: row r's extra pieces are [first[r], first[r + 1])
    std::vector<int32_t> piece_row;   // per extra piece: its row ...
    std::vector<int64_t> piece_p0;    // ... and its links [p0, p1) of the raw list
    std::vector<int64_t> piece_p1;
    bool too_many = false;            // more than INT32_MAX pieces (a raw list of > 2^40 links): nothing is planned
};

inline AudLongRows aud_long_rows(int32_t n, const int64_t *rowptr)
{
    AudLongRows L;
    L.first.push_back(0);
    int64_t total = 0;
    for (int32_t i = 0; i < n; ++i) total += aud_extra_pieces(rowptr[i + 1] - rowptr[i]);
    if (total > 0x7FFFFFFFll) { L.too_many = true; return L; }
    for (int32_t i = 0; i < n; ++i) {
        const int64_t p0 = rowptr[i], p1 = rowptr[i + 1], extra = aud_extra_pieces(p1 - p0);
        if (extra == 0) continue;
        L.row.push_back(i);
        for (int64_t q = 1; q <= extra; ++q) {
            const int64_t a = p0 + q * AUD_SPLIT, b = a + AUD_SPLIT;
            L.piece_row.push_back(i);
            L.piece_p0.push_back(a);
            L.piece_p1.push_back(b < p1 ? b : p1);
        }
        L.first.push_back((int32_t)L.piece_row.size());
    }
    return L;
}

// ---- the target-to-column table of the in-link exclusion -----------------------------------------------------------------------
// slot_target[q]: the target in slot q of the call (-1: padding); slots_per_group slots form a tile group.  Per group the
// distinct targets ascending, each with the group-local slots that hold it (ascending): a target that repeats in the batch
// owns several columns.  node[group_off[grp] .. group_off[grp + 1]) are the group's targets; entry e owns
// slot[ptr[e] .. ptr[e + 1]).
struct AudTargets {
    std::vector<int64_t> group_off;
    std::vector<int32_t> node;
    std::vector<int32_t> ptr;         // node.size() + 1
    std::vector<int32_t> slot;
};

inline AudTargets aud_targets(size_t nslots, const int32_t *slot_target, size_t slots_per_group)
{
    AudTargets t;
    t.group_off.push_back(0);
    t.ptr.push_back(0);
    if (slots_per_group == 0) return t;
    std::vector<std::pair<int32_t, int32_t>> pairs;
    for (size_t q0 = 0; q0 < nslots; q0 += slots_per_group) {
        const size_t q1 = q0 + slots_per_group < nslots ? q0 + slots_per_group : nslots;
        pairs.clear();
        for (size_t q = q0; q < q1; ++q)
            if (slot_target[q] >= 0) pairs.emplace_back(slot_target[q], (int32_t)(q - q0));
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

// the entry of `node` among the sorted targets tn[0 .. cnt), or -1: what k_audience_exclude runs per masked link whose
// target has its bit in the group's bitmap
RWR_AUD_HD inline int32_t aud_target_find(const int32_t *tn, int32_t cnt, int32_t node)
{
    int32_t lo = 0, hi = cnt;
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo) / 2;
        if (tn[mid] < node) lo = mid + 1;
        else hi = mid;
    }
    return lo < cnt && tn[lo] == node ? lo : -1;
}

// the source row of raw link p: the last row i with rowptr[i] <= p (rows without links are skipped by the search itself)
RWR_AUD_HD inline int32_t aud_link_row(const int64_t *rowptr, int32_t n, int64_t p)
{
    int32_t lo = 0, hi = n;             // invariant: rowptr[lo] <= p < rowptr[hi]
    while (hi - lo > 1) {
        const int32_t mid = lo + (hi - lo) / 2;
        if (rowptr[mid] <= p) lo = mid;
        else hi = mid;
    }
    return lo;
}

// ---- workspace sizes, in elements, in 64-bit arithmetic --------------------------------------------------------------------------
// one [tile][n][G] matrix of a group of tg tiles (the accumulator and each of the two g buffers)
inline uint64_t aud_mat_elems(int tg, int32_t n, int G) { return (uint64_t)(tg > 0 ? tg : 0) * (uint64_t)n * (uint64_t)G; }
// the T x n table of rho, and the T x n table of h beside it while rho is built; nothing on a graph without dangling nodes
inline uint64_t aud_rho_elems(int64_t T, int32_t n, bool any_dangling) { return any_dangling && T > 0 ? (uint64_t)T * (uint64_t)n : 0; }
// the partial sums of a step's extra pieces: [piece][tile][G]
inline uint64_t aud_part_elems(uint64_t pieces, int tg, int G) { return pieces * (uint64_t)(tg > 0 ? tg : 0) * (uint64_t)G; }

// ---- the restart mass of one node ------------------------------------------------------------------------------------------
// rho_k = d n + (1 - d) delta_k, delta_k = n h_k + sum_{m < k} rho_m h_{k-1-m}: the mass a walk from this node holds on dangling
// nodes after k steps, from h_j = its column of B^j applied to the dangling indicator.  Element k of h / rho lies k * stride
// further.  Every product and every sum is rounded on its own, in the order written here (no FMA: the library is built with
// -ffp-contract=off), m ascending -- k_rev_rho is this function.
RWR_AUD_HD inline void aud_rho_node(int32_t n, double d, int32_t T, const double *h, size_t h_stride, double *rho, size_t rho_stride)
{
    const double nn = (double)n, dn = d * nn, c1 = 1 - d;
    for (int32_t k = 0; k < T; ++k) {
        double delta = nn * h[(size_t)k * h_stride];
        for (int32_t m = 0; m < k; ++m) {
            const double t = rho[(size_t)m * rho_stride] * h[(size_t)(k - 1 - m) * h_stride];
            delta = delta + t;
        }
        const double r = c1 * delta;
        rho[(size_t)k * rho_stride] = dn + r;
    }
}

}  // namespace rwr
