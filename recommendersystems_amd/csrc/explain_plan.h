// What one rwr_recommend_explained_batch call decides on the host about its reasons: the sizes of its extra
// tables, and a host model of the selection explain.hip carries out per list entry -- the best n_why in-link addends by
// (value bits descending, in-list position ascending) and the number of positive addends.  (The verdict on the arguments is
// typed_call.h's.)  Plain C++17 without HIP (the functions the kernel shares carry WHY_HD), so that
// tests/cpp/explain_plan_check.cpp checks all of it against brute-force loops on the host.
//
// The reasons of list entry v of a column: in-entry e (position e of v's in-list, the addend order of Model.deliverRanks)
// has the addend a_e = fl(fl(c1 * y[u_e]) * w_e) -- why_addend() -- and is a reason iff a_e > 0.  Addends are >= +0.0, so
// their bit patterns order as unsigned integers and bits == 0 says "no reason".  On the device the lanes of a workgroup
// stride the in-list, each keeps a WhyList of its own entries, and the lists are merged (why_list_merge) lane to lane and
// wave to wave; the best n_why of a union do not depend on the order of the merges, because the key (bits, position) is
// total.  why_select() is that procedure with the lane count as a parameter.
#pragma once

#include <cstddef>
#include <cstdint>

#include "cap_plan.h"

#if defined(__HIPCC__)
#define WHY_HD __host__ __device__ __forceinline__
#else
#define WHY_HD inline
#endif

namespace rwr {

constexpr int32_t WHY_MAX = 8;          // == RWR_WHY_MAX (explain.hip asserts it): slots of a lane's list, in registers

// ---- the addend and its key ----------------------------------------------------------------------------------------------------
// the two products rounded separately (Model.cs:84, 87; the library is built without FMA contraction, and there is no add)
WHY_HD double why_addend(double c1, double y, double w)
{
    const double rw = c1 * y;
    return rw * w;
}
WHY_HD uint64_t why_bits(double a)
{
    uint64_t u;
    __builtin_memcpy(&u, &a, 8);
    return u;
}
WHY_HD double why_value(uint64_t bits)
{
    double a;
    __builtin_memcpy(&a, &bits, 8);
    return a;
}
// a reason: a positive addend (not +0.0, not -0.0, not a NaN; the ranked entries' domain has none below zero)
WHY_HD bool why_is_reason(double a) { return a > 0.0; }

// bits = the addend's pattern, pos = its in-list position.  {0, ~0} is "empty" and lies below every reason, {~0, 0} above
struct WhyKey {
    uint64_t bits;
    uint32_t pos;
};
WHY_HD bool why_better(const WhyKey &a, const WhyKey &b) { return a.bits != b.bits ? a.bits > b.bits : a.pos < b.pos; }
WHY_HD bool why_is_top(const WhyKey &a) { return a.bits == ~0ull; }
WHY_HD bool why_is_empty(const WhyKey &a) { return a.bits == 0; }

// A list: slots [WHY_MAX - r, WHY_MAX) hold the best r keys seen, descending, empty where fewer were seen; the slots in front
// of them hold the top sentinel, which nothing passes -- so no slot is ever addressed by a run-time index (cap_plan.h's
// CapList, with another key).  r == 0: every slot is a sentinel and nothing is ever kept.
struct WhyList {
    WhyKey k[WHY_MAX];
};
WHY_HD void why_list_init(WhyList &l, int32_t r)
{
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < WHY_MAX; ++j) l.k[j] = j < WHY_MAX - r ? WhyKey{~0ull, 0u} : WhyKey{0ull, ~0u};
}
WHY_HD void why_list_insert(WhyList &l, const WhyKey &key)
{
    if (!why_better(key, l.k[WHY_MAX - 1])) return;
    l.k[WHY_MAX - 1] = key;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = WHY_MAX - 1; j > 0; --j)
        if (why_better(l.k[j], l.k[j - 1])) {
            const WhyKey t = l.k[j];
            l.k[j] = l.k[j - 1];
            l.k[j - 1] = t;
        }
}
// the reasons of another list over OTHER in-entries join this one
WHY_HD void why_list_merge(WhyList &l, const WhyList &other)
{
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < WHY_MAX; ++j)
        if (!why_is_top(other.k[j]) && !why_is_empty(other.k[j])) why_list_insert(l, other.k[j]);
}

// The selection over one in-list as the kernel computes it: `lanes` lanes stride the `deg` entries (lane l takes positions
// l, l + lanes, ...), the lanes' lists are merged in a butterfly (lanes a power of two).  y(e) / w(e): the source's previous
// rank and the normalised weight of in-entry e.  out_pos / out_bits: r cells, unused ones UINT32_MAX / 0.  Returns why_total.
template <class Y, class W>
inline int64_t why_select(int64_t deg, double c1, Y &&y, W &&w, int32_t r, int32_t lanes, uint32_t *out_pos, uint64_t *out_bits)
{
    int64_t total = 0;
    WhyList *ls = new WhyList[(size_t)lanes];
    for (int32_t l = 0; l < lanes; ++l) {
        why_list_init(ls[l], r);
        for (int64_t e = l; e < deg; e += lanes) {
            const double a = why_addend(c1, y(e), w(e));
            if (!why_is_reason(a)) continue;
            ++total;
            why_list_insert(ls[l], WhyKey{why_bits(a), (uint32_t)e});
        }
    }
    for (int32_t o = lanes >> 1; o > 0; o >>= 1)
        for (int32_t l = 0; l < lanes; ++l)
            if ((l & o) == 0) {                                  // (both partners end with the same list: keep one)
                why_list_merge(ls[l], ls[l ^ o]);
                ls[l ^ o] = ls[l];
            }
    for (int32_t i = 0; i < r; ++i) {
        const WhyKey &k = ls[0].k[WHY_MAX - r + i];
        out_pos[i] = why_is_empty(k) ? ~0u : k.pos;
        out_bits[i] = why_is_empty(k) ? 0 : k.bits;
    }
    delete[] ls;
    return total;
}

// ---- the tables -----------------------------------------------------------------------------------------------------------------
// nodes and why_total: K x top_n cells; why_src and why_term: K x top_n x n_why, entry (k, j)'s cells from why_offset on
inline size_t why_entry_cells(int32_t K, int32_t top_n) { return (size_t)K * (size_t)top_n; }
inline size_t why_reason_cells(int32_t K, int32_t top_n, int32_t n_why) { return why_entry_cells(K, top_n) * (size_t)n_why; }
WHY_HD size_t why_offset(int32_t k, int32_t j, int32_t top_n, int32_t n_why) { return ((size_t)k * (size_t)top_n + (size_t)j) * (size_t)n_why; }

}  // namespace rwr
