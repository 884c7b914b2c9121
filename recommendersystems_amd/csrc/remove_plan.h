// Which links of one rwr_graph_remove_links call leave the resident raw lists and where the others go, decided
// by remove_plan() from the handle's host row pointers and the call's positions alone and carried out by graph_remove
// (remove.hip).  Plain C++17 without HIP, so that tests/cpp/remove_plan_check.cpp checks it against a list-of-lists erase on
// the host; the index arithmetic of the device kernels (rm_* below) is __host__ __device__ and runs in that program as well.
//
// Let r[0] < r[1] < ... be the removed positions ascending.  The flat list is the concatenation of the rows and erasing keeps
// the order of everything else, so the surviving old position e moves DOWN by the removed positions in front of it:
//     shift(e) = #{k : r[k] < e} = lower_bound(r, e),        new position = e - shift(e)
// -- a step function of e with one step behind every removed position.  On the survivors e - shift(e) is strictly increasing
// (between two survivors e < e' lie at most e' - e - 1 removed positions) and takes every value of [0, m_old - count) once.
// A row pointer is a position as well: rowptr_new[i] = rowptr_old[i] - lower_bound(r, rowptr_old[i]), the removed links of
// the rows before i.  The table has one entry per removed link: O(count), never O(n) or O(m).
#pragma once

#include <algorithm>
#include <cstdint>
#include <numeric>
#include <vector>

#if defined(__HIPCC__)
#define RMP_HD __host__ __device__
#else
#define RMP_HD
#endif

namespace rwr {

// ---- what the device kernels compute per row pointer and per chunk of old positions (remove.hip)
constexpr int RM_CHUNK = 8192;     // old positions per workgroup
// More removed positions than this in a chunk: the dense path of k_remove_compact (per-element shifts).  The value is §3.11's,
// by the same reasoning and as little tuned: a segment is walked by all 256 lanes, so segments under 256 elements leave lanes
// idle in every one of the three block copies, and 8 192 / 32 = 256 is the average segment length at which that starts.
constexpr int RM_DENSE_REMOVED = 32;

// first k in [lo, hi) with r[k] >= v (hi if there is none)
RMP_HD inline int64_t rm_lower_bound(const int64_t *r, int64_t lo, int64_t hi, int64_t v)
{
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (r[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

RMP_HD inline int64_t rm_rowptr_new(const int64_t *r, int64_t nr, int64_t rowptr_old_i)
{
    return rowptr_old_i - rm_lower_bound(r, 0, nr, rowptr_old_i);
}

// the removed positions inside the chunk [c0, c1) of old positions: r[j .. jend); r[0 .. j) lie in front of the chunk
struct RmSlice { int64_t j, jend; };
RMP_HD inline RmSlice rm_chunk_slice(const int64_t *r, int64_t nr, int64_t c0, int64_t c1)
{
    RmSlice s;
    s.j = rm_lower_bound(r, 0, nr, c0);
    s.jend = rm_lower_bound(r, s.j, nr, c1);
    return s;
}
RMP_HD inline bool rm_chunk_dense(RmSlice s) { return s.jend - s.j > RM_DENSE_REMOVED; }

// Sparse path: the chunk's survivors are the segments between its removed positions, number t = 0 .. jend - j.  Segment t
// starts behind r[j + t - 1] (the chunk's start for t = 0), ends before r[j + t] (the chunk's end for the last one) and has
// j + t removed positions in front of it: old positions [a, b) go to [a - sh, b - sh).  Neighbouring removed positions
// leave an empty segment (a == b).
struct RmSeg { int64_t a, b, sh; };
RMP_HD inline RmSeg rm_segment(const int64_t *r, RmSlice s, int64_t c0, int64_t c1, int64_t t)
{
    RmSeg g;
    g.a = t == 0 ? c0 : r[s.j + t - 1] + 1;
    g.b = s.j + t == s.jend ? c1 : r[s.j + t];
    g.sh = s.j + t;
    return g;
}

// Dense path: the old position e of the chunk; false if it is a removed one, else its new position.  r[0 .. j) < c0 <= e and
// r[jend ..) >= c1 > e, so the bisection of the chunk's own slice is the global lower_bound(r, e).
RMP_HD inline bool rm_dense_dest(const int64_t *r, RmSlice s, int64_t e, int64_t *dest)
{
    const int64_t k = rm_lower_bound(r, s.j, s.jend, e);
    if (k < s.jend && r[k] == e) return false;
    *dest = e - k;
    return true;
}

// ---- the host plan
enum RemoveVerdict : int32_t {
    REMOVE_OK = 0,
    REMOVE_BAD_RANGE = 1,    // link_index[bad_q] outside [0, m_old)
    REMOVE_DUPLICATE = 2,    // link_index[bad_q] equals an earlier entry (bad_q is the second occurrence)
};

struct RemovePlan {
    RemoveVerdict verdict = REMOVE_OK;
    int64_t bad_q = -1;
    int64_t m_old = 0, m_new = 0;
    std::vector<int64_t> r;            // [count] the removed positions ascending
    std::vector<int64_t> rowptr_new;   // [n + 1]

    // how far DOWN the surviving old position e moves
    int64_t shift(int64_t e) const { return rm_lower_bound(r.data(), 0, (int64_t)r.size(), e); }
};

// The entries q in [0, count) stably by position: a least-significant-digit radix sort, 11 bits of link_index[q] a pass (one
// pass up to 2 048 links, two up to 4 M, three up to the build's limit of 2^32-2).  O(count) a pass, where a comparison sort
// that reads the positions through the permutation is not (append_plan.h: append_order_by_source measured it).  Every pass is
// a counting sort, which keeps equal digits in their order: equal positions stay in the order of q, which is how the plan
// names the SECOND occurrence of a duplicate.  link_index[q] in [0, m_old) is the caller's check.
inline void remove_order_by_position(int64_t m_old, int64_t count, const int64_t *link_index, std::vector<int64_t> &order)
{
    constexpr int BITS = 11;
    constexpr int64_t MASK = (1 << BITS) - 1;
    order.resize((size_t)(count > 0 ? count : 0));
    std::iota(order.begin(), order.end(), (int64_t)0);
    if (count < 2) return;
    std::vector<int64_t> other((size_t)count), head((size_t)MASK + 1);
    for (int sh = 0; sh < 63 && ((m_old - 1) >> sh) > 0; sh += BITS) {
        std::fill(head.begin(), head.end(), (int64_t)0);
        for (int64_t k = 0; k < count; ++k) ++head[(size_t)((link_index[order[(size_t)k]] >> sh) & MASK)];
        int64_t at = 0;
        for (int64_t &h : head) { const int64_t c = h; h = at; at += c; }
        for (int64_t k = 0; k < count; ++k) {
            const int64_t q = order[(size_t)k];
            other[(size_t)head[(size_t)((link_index[q] >> sh) & MASK)]++] = q;
        }
        order.swap(other);
    }
}

// rowptr: the n + 1 row pointers of the resident raw lists.  Validation comes first and looks at every entry before anything
// is planned: the first position out of range, else the first entry that repeats an earlier one.
inline RemovePlan remove_plan(int32_t n, const int64_t *rowptr, int64_t count, const int64_t *link_index)
{
    RemovePlan p;
    p.m_old = p.m_new = rowptr[n];
    if (count < 0) count = 0;
    for (int64_t q = 0; q < count; ++q)
        if (link_index[q] < 0 || link_index[q] >= p.m_old) { p.verdict = REMOVE_BAD_RANGE; p.bad_q = q; return p; }

    std::vector<int64_t> order;
    remove_order_by_position(p.m_old, count, link_index, order);
    for (int64_t k = 0; k + 1 < count; ++k) {
        const int64_t q2 = order[(size_t)k + 1];           // (stable: behind an equal position stands the later q)
        if (link_index[order[(size_t)k]] == link_index[q2] && (p.bad_q < 0 || q2 < p.bad_q)) p.bad_q = q2;
    }
    if (p.bad_q >= 0) { p.verdict = REMOVE_DUPLICATE; return p; }

    p.m_new = p.m_old - count;
    p.r.resize((size_t)count);
    for (int64_t k = 0; k < count; ++k) p.r[(size_t)k] = link_index[order[(size_t)k]];
    // one merge walk of the row pointers (non-decreasing) and r: k = the removed positions in front of rowptr[i]
    p.rowptr_new.resize((size_t)n + 1);
    int64_t k = 0;
    for (int64_t i = 0; i <= n; ++i) {
        while (k < count && p.r[(size_t)k] < rowptr[i]) ++k;
        p.rowptr_new[(size_t)i] = rowptr[i] - k;
    }
    return p;
}

}  // namespace rwr
