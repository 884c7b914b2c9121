// Where the links of one rwr_graph_append_links call go, decided by append_plan() from the handle's host row
// pointers and the call's src / dst arrays alone and carried out by graph_append (append.hip).  Plain C++17 without HIP,
// so that tests/cpp/append_plan_check.cpp checks it against a list-of-lists append on the host.
//
// Link q goes to the END of row src[q]; links of one row keep the order of q.  Let the distinct sources be s_0 < s_1 < ... with
// c_j appended links each.  Everything that followed row s_j in the old flat list moves up by c_j, so the old position e moves by
//     shift(e) = sum of c_j over the j with rowptr_old[s_j + 1] <= e
// -- a step function of e whose steps ("breakpoints") are brk[j] = rowptr_old[s_j + 1], non-decreasing in j.  Rows without
// links between two sources only make breakpoints coincide; the sum over "<= e" takes all of them.  With cum[j] = c_0 + ... +
// c_j the shift is cum[upper_bound(brk, e) - 1] (0 before the first breakpoint), the new row pointer of row i is
// rowptr_old[i] + cum[lower_bound(srcs, i) - 1] (the appended links with src < i), and the r-th link appended to s_j lands at
// brk[j] + (cum[j] - c_j) + r.  The tables have one entry per DISTINCT source: O(count), never O(n) or O(m).
//
// The index arithmetic of the device kernels (ap_* below) is __host__ __device__ and runs in that program as well, chunk by
// chunk through both of the merge kernel's paths.
#pragma once

#include <algorithm>
#include <cstdint>
#include <numeric>
#include <vector>

#if defined(__HIPCC__)
#define APP_HD __host__ __device__
#else
#define APP_HD
#endif

namespace rwr {

// ---- what the device kernels compute per row pointer and per chunk of old positions (append.hip)
constexpr int AP_CHUNK = 8192;     // old positions per workgroup
// More breakpoints than this in a chunk: the dense path of k_append_merge (per-element shifts).  The value is reasoned, not
// tuned: a segment is walked by all 256 lanes, so segments under 256 elements leave lanes idle in every one of the three block
// copies, and 8 192 / 32 = 256 is the average segment length at which that starts.  A bisection over at most 8 192 breakpoints
// of the chunk costs each element up to 13 uniform-ish loads from a table the whole workgroup keeps in cache.
constexpr int AP_DENSE_BREAKS = 32;

// first k in [0, nb) with srcs[k] >= i (nb if there is none): the distinct sources below row i
APP_HD inline int ap_sources_below(const int32_t *srcs, int nb, int64_t i)
{
    int lo = 0, hi = nb;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if ((int64_t)srcs[mid] < i) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
// first k in [lo, hi) with brk[k] > v (hi if there is none)
APP_HD inline int ap_upper_bound(const int64_t *brk, int lo, int hi, int64_t v)
{
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (brk[mid] <= v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// rowptr_new[i] = rowptr_old[min(i, n_old)] + (appended links with src < i), i in [0, n]: the rows past n_old are the call's
// new nodes, whose lists were empty before it (rowptr_old has n_old + 1 entries)
APP_HD inline int64_t ap_rowptr_new(const int32_t *srcs, const int64_t *cum, int nb, const int64_t *rowptr_old, int32_t n_old,
                                    int64_t i)
{
    const int k = ap_sources_below(srcs, nb, i);
    return rowptr_old[i < n_old ? i : (int64_t)n_old] + (k > 0 ? cum[k - 1] : 0);
}

// the breakpoints inside the chunk [c0, c1) of old positions, c0 < c1: brk[j .. jend) lie in (c0, c1 - 1]; brk[0 .. j) <= c0
// have moved the whole chunk already, brk[jend ..) >= c1 move nothing of it
struct ApSlice { int j, jend; };
APP_HD inline ApSlice ap_chunk_slice(const int64_t *brk, int nb, int64_t c0, int64_t c1)
{
    ApSlice s;
    s.j = ap_upper_bound(brk, 0, nb, c0);
    s.jend = ap_upper_bound(brk, s.j, nb, c1 - 1);
    return s;
}
APP_HD inline bool ap_chunk_dense(ApSlice s) { return s.jend - s.j > AP_DENSE_BREAKS; }

// Sparse path: the segment of the chunk that starts at old position a, where j is the first breakpoint behind a (brk[j] > a;
// for a = c0 that is the slice's j).  Old positions [a, b) move up by sh; the walk goes on at a = b with j = next, which has
// skipped every breakpoint equal to b (coinciding ones: sources that are neighbouring rows without links), until b == c1.
struct ApSeg { int64_t a, b, sh; int next; };
APP_HD inline ApSeg ap_segment(const int64_t *brk, const int64_t *cum, int nb, int64_t c1, int64_t a, int j)
{
    ApSeg g;
    g.a = a;
    g.sh = j > 0 ? cum[j - 1] : 0;
    g.b = (j < nb && brk[j] < c1) ? brk[j] : c1;
    while (j < nb && brk[j] <= g.b) ++j;
    g.next = j;
    return g;
}

// Dense path: the new position of the old position e of the chunk.  brk[0 .. j) <= c0 <= e and brk[jend ..) > e, so the
// bisection of the chunk's own slice is the global upper_bound(brk, e).
APP_HD inline int64_t ap_dense_dest(const int64_t *brk, const int64_t *cum, ApSlice s, int64_t e)
{
    const int k = ap_upper_bound(brk, s.j, s.jend, e);
    return e + (k > 0 ? cum[k - 1] : 0);
}

// ---- the host plan

constexpr int64_t APPEND_MAX_LINKS = 0xFFFFFFFEll;   // the build's per-device limit of 2^32-2 links (build.hip: graph_build_upload)

enum AppendVerdict : int32_t {
    APPEND_OK = 0,
    APPEND_BAD_SRC = 1,      // src[bad_q] outside [0, n)
    APPEND_BAD_DST = 2,      // dst[bad_q] outside [0, n)
    APPEND_TOO_MANY = 3,     // nnz_raw + count beyond APPEND_MAX_LINKS
};

struct AppendPlan {
    AppendVerdict verdict = APPEND_OK;
    int64_t bad_q = -1;               // the first offending entry (BAD_SRC / BAD_DST)
    int64_t m_old = 0, m_new = 0;
    std::vector<int64_t> order;       // [count] the entries q, stably by source: order[k] is the k-th appended link in list order
    std::vector<int32_t> srcs;        // [distinct] sources ascending
    std::vector<int64_t> cnt;         // [distinct] links appended to srcs[j]
    std::vector<int64_t> brk;         // [distinct] rowptr_old[srcs[j] + 1]: old positions >= brk[j] move by cnt[j] more
    std::vector<int64_t> cum;         // [distinct] cnt[0] + ... + cnt[j]
    std::vector<int64_t> pos;         // [count] new flat position of link order[k]
    std::vector<int64_t> new_index;   // [count] new flat position of link q (new_index[order[k]] = pos[k])

    // how far the old flat position e moves
    int64_t shift(int64_t e) const
    {
        const size_t j = (size_t)(std::upper_bound(brk.begin(), brk.end(), e) - brk.begin());
        return j == 0 ? 0 : cum[j - 1];
    }
    // the appended links with src < i: what rowptr[i] grows by (i in [0, n])
    int64_t row_shift(int64_t i) const
    {
        const size_t j = (size_t)(std::lower_bound(srcs.begin(), srcs.end(), i,
                                                   [](int32_t s, int64_t v) { return (int64_t)s < v; }) - srcs.begin());
        return j == 0 ? 0 : cum[j - 1];
    }
};

// The entries q in [0, count) stably by source: a least-significant-digit radix sort, 11 bits of src[q] a pass (one pass up to
// 2 048 nodes, two up to 4 M, three beyond).  Every pass is a counting sort, which keeps equal digits in their order, so links
// of one source stay in the order of q.  O(count) a pass: a comparison sort that reads src through the permutation took 5.5 ms
// of a 100 000-link call, more than the device work of the whole append.  src[q] in [0, n) is the caller's check.
inline void append_order_by_source(int32_t n, int64_t count, const int32_t *src, std::vector<int64_t> &order)
{
    constexpr int BITS = 11;
    constexpr int32_t MASK = (1 << BITS) - 1;
    order.resize((size_t)count);
    std::iota(order.begin(), order.end(), (int64_t)0);
    if (count < 2) return;
    std::vector<int64_t> other((size_t)count), head((size_t)MASK + 1);
    for (int sh = 0; sh < 31 && ((n - 1) >> sh) > 0; sh += BITS) {
        std::fill(head.begin(), head.end(), (int64_t)0);
        for (int64_t k = 0; k < count; ++k) ++head[(size_t)((src[order[(size_t)k]] >> sh) & MASK)];
        int64_t at = 0;
        for (int64_t &h : head) { const int64_t c = h; h = at; at += c; }
        for (int64_t k = 0; k < count; ++k) {
            const int64_t q = order[(size_t)k];
            other[(size_t)head[(size_t)((src[q] >> sh) & MASK)]++] = q;
        }
        order.swap(other);
    }
}

// rowptr: the n + 1 row pointers of the resident raw lists.  Validation comes first and looks at every entry before anything
// is planned: the first bad src, else the first bad dst, else the link limit.
inline AppendPlan append_plan(int32_t n, const int64_t *rowptr, int64_t count, const int32_t *src, const int32_t *dst)
{
    AppendPlan p;
    p.m_old = rowptr[n];
    p.m_new = p.m_old + (count > 0 ? count : 0);
    for (int64_t q = 0; q < count; ++q)
        if (src[q] < 0 || src[q] >= n) { p.verdict = APPEND_BAD_SRC; p.bad_q = q; return p; }
    for (int64_t q = 0; q < count; ++q)
        if (dst[q] < 0 || dst[q] >= n) { p.verdict = APPEND_BAD_DST; p.bad_q = q; return p; }
    if (count > 0 && (p.m_old > APPEND_MAX_LINKS || count > APPEND_MAX_LINKS - p.m_old)) { p.verdict = APPEND_TOO_MANY; return p; }
    if (count <= 0) return p;

    append_order_by_source(n, count, src, p.order);
    p.pos.resize((size_t)count);
    p.new_index.resize((size_t)count);
    int64_t before = 0;               // links appended to smaller sources
    for (int64_t k = 0; k < count;) {
        const int32_t s = src[p.order[(size_t)k]];
        int64_t k1 = k;
        while (k1 < count && src[p.order[(size_t)k1]] == s) ++k1;
        const int64_t b = rowptr[(size_t)s + 1];
        for (int64_t r = k; r < k1; ++r) {
            p.pos[(size_t)r] = b + before + (r - k);
            p.new_index[(size_t)p.order[(size_t)r]] = p.pos[(size_t)r];
        }
        before += k1 - k;
        p.srcs.push_back(s);
        p.cnt.push_back(k1 - k);
        p.brk.push_back(b);
        p.cum.push_back(before);
        k = k1;
    }
    return p;
}

}  // namespace rwr
