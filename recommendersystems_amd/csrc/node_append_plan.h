// Where the nodes of one rwr_graph_append_nodes call go: the grown host row pointers and the two ITEM orders,
// decided here and carried out by graph_append (append.hip).  Plain C++17; the two position functions also compile as
// device code, so that k_item_order_merge and tests/cpp/node_append_plan_check.cpp run the same bisections.
//
// Row pointers.  New node j is row n_old + j with an empty list: rowptr_ext[i] = rowptr_old[n_old] for i in (n_old, n_total].
// The links of the call are then planned by append_plan() over n_total rows of that extended array, unchanged.
//
// item_rows (ITEM rows by row index ascending): the new ITEM rows are larger than every resident row, so they go to its end.
//
// item_order (ITEM rows by id descending).  rwr_graph_create sorts the keys top - orderable(id) ascending with a STABLE radix
// sort whose input is item_rows, i.e. row-ascending (build.hip: k_item_id_keys and the sort behind it).  THE TIE RULE: ITEM
// rows of equal id stand in row-ascending order, so a resident row stands before a new row of the same id, and new rows of
// equal id keep the order of the call.  The grown order is therefore the stable merge of
//     A = the resident item_order                    (ids descending, ties row-ascending), with
//     B = the new ITEM rows stably by id descending  (node_append_sort_new),
// where A wins ties:
//     A[q] moves to q + #{r : id(B[r]) >  id(A[q])}      (nap_old_dest)
//     B[r] goes  to r + #{q : id(A[q]) >= id(B[r])}      (nap_new_dest)
// -- one bisection in the OTHER list per element, no re-sort of the resident items.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "key_bits.h"

#if defined(__HIPCC__)
#define NAP_HD __host__ __device__
#else
#define NAP_HD
#endif

namespace rwr {

// the order-preserving unsigned form of an id (common.h: i64_orderable)
NAP_HD inline uint64_t nap_orderable(int64_t id) { return (uint64_t)id ^ 0x8000000000000000ull; }

// first position p of [0, len) with !(before(p)); before() is true on a prefix
template <class Pred>
NAP_HD inline int32_t nap_partition_point(int32_t len, Pred before)
{
    int32_t lo = 0, hi = len;
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (before(mid)) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// Destination of resident entry q of item_order.  id_new(r) = the id of B[r], descending in r.
template <class IdNew>
NAP_HD inline int32_t nap_old_dest(int32_t q, int64_t id_q, int32_t n_new_items, IdNew id_new)
{
    const uint64_t k = nap_orderable(id_q);
    return q + nap_partition_point(n_new_items, [&](int32_t r) { return nap_orderable(id_new(r)) > k; });
}
// Destination of new entry r.  id_old(q) = the id of A[q], descending in q.
template <class IdOld>
NAP_HD inline int32_t nap_new_dest(int32_t r, int64_t id_r, int32_t n_old_items, IdOld id_old)
{
    const uint64_t k = nap_orderable(id_r);
    return r + nap_partition_point(n_old_items, [&](int32_t q) { return nap_orderable(id_old(q)) >= k; });
}

enum NodeAppendVerdict : int32_t {
    NODE_APPEND_OK = 0,
    NODE_APPEND_TOO_MANY = 1,    // n_old + n_new beyond INT32_MAX
};

struct NodeAppendPlan {
    NodeAppendVerdict verdict = NODE_APPEND_OK;
    int32_t n_old = 0, n_total = 0;
    int32_t n_new_items = 0;
    std::vector<int32_t> new_item_rows;     // [n_new_items] the new ITEM rows ascending: the tail of item_rows
    std::vector<int32_t> new_item_sorted;   // [n_new_items] ... stably by id descending: B
    // range of the new ITEM ids in the order-preserving form (valid when n_new_items > 0)
    uint64_t key_lo = ~0ull, key_hi = 0;
};

// rows (ascending) stably by id descending: a least-significant-digit radix sort of key_hi - orderable(id), 11 bits a pass over
// the bits the id RANGE needs (consecutive ids of a loader: two passes for 100 000 items).  Every pass is a counting sort,
// which keeps equal digits in their order.  id_of(row) = the id of a row in `rows`.
template <class IdOf>
inline void node_append_sort_new(std::vector<int32_t> &rows, uint64_t key_lo, uint64_t key_hi, IdOf id_of)
{
    constexpr int BITS = 11;
    constexpr uint64_t MASK = (1u << BITS) - 1;
    const size_t cnt = rows.size();
    if (cnt < 2) return;
    const int bits = bit_length(key_hi - key_lo);
    std::vector<uint64_t> key(cnt), key2(cnt);
    std::vector<int32_t> other(cnt);
    std::vector<size_t> head((size_t)MASK + 1);
    for (size_t k = 0; k < cnt; ++k) key[k] = key_hi - nap_orderable(id_of(rows[k]));
    for (int sh = 0; sh < bits; sh += BITS) {
        std::fill(head.begin(), head.end(), (size_t)0);
        for (size_t k = 0; k < cnt; ++k) ++head[(size_t)((key[k] >> sh) & MASK)];
        size_t at = 0;
        for (size_t &h : head) { const size_t c = h; h = at; at += c; }
        for (size_t k = 0; k < cnt; ++k) {
            const size_t to = head[(size_t)((key[k] >> sh) & MASK)]++;
            other[to] = rows[k];
            key2[to] = key[k];
        }
        rows.swap(other);
        key.swap(key2);
    }
}

// node_id / node_type: the n_new nodes of the call; item_type: the type value of an ITEM node
inline NodeAppendPlan node_append_plan(int32_t n_old, int32_t n_new, const int64_t *node_id, const uint8_t *node_type,
                                       uint8_t item_type)
{
    NodeAppendPlan p;
    p.n_old = n_old;
    p.n_total = n_old;
    if (n_new > 0 && (int64_t)n_old + (int64_t)n_new > (int64_t)INT32_MAX) { p.verdict = NODE_APPEND_TOO_MANY; return p; }
    if (n_new <= 0) return p;
    p.n_total = n_old + n_new;
    for (int32_t j = 0; j < n_new; ++j)
        if (node_type[j] == item_type) {
            p.new_item_rows.push_back(n_old + j);
            const uint64_t k = nap_orderable(node_id[j]);
            p.key_lo = k < p.key_lo ? k : p.key_lo;
            p.key_hi = k > p.key_hi ? k : p.key_hi;
        }
    p.n_new_items = (int32_t)p.new_item_rows.size();
    p.new_item_sorted = p.new_item_rows;
    node_append_sort_new(p.new_item_sorted, p.key_lo, p.key_hi, [&](int32_t row) { return node_id[row - n_old]; });
    return p;
}

// rwr_graph_create's sort-key parameters of the ITEM ids (build.hip: graph_build_upload) for an id range [lo, hi] in the
// order-preserving form; no item: top 0, one bit
inline void node_append_id_keys(bool any, uint64_t lo, uint64_t hi, uint64_t *top, int32_t *bits)
{
    *top = any ? hi : 0;
    *bits = any ? key_bits(hi - lo) : 1;
}

// the host row pointers grown to n_total rows (the new rows are empty); capacity for them must not be a surprise to the
// caller: std::vector::resize gives the strong guarantee, so a failed growth leaves rp as it was
inline void node_append_extend_rowptr(std::vector<int64_t> &rp, int32_t n_old, int32_t n_total)
{
    const int64_t m_old = rp[(size_t)n_old];
    rp.resize((size_t)n_total + 1, m_old);
}

// rp[i] += appended links with src < i, i in [0, n_total]: srcs ascending and distinct, cum their running link counts
// (AppendPlan::srcs / cum)
inline void node_append_shift_rowptr(std::vector<int64_t> &rp, int32_t n_total, const std::vector<int32_t> &srcs,
                                     const std::vector<int64_t> &cum)
{
    const size_t nb = srcs.size();
    size_t j = 0;
    for (int32_t i = 0;; ++i) {
        while (j < nb && srcs[j] < i) ++j;
        rp[(size_t)i] += j > 0 ? cum[j - 1] : 0;
        if (i == n_total) break;
    }
}

}  // namespace rwr
