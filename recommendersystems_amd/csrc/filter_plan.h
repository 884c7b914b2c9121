// What one rwr_recommend_filtered_batch / rwr_recommend_filtered_positions_batch call decides on the host: the
// verdict on its arguments, and the geometry of the device-side build of its candidate list from the caller's pool -- carried
// out by filter.hip.  Plain C++17 without HIP, so that tests/cpp/filter_plan_check.cpp checks both against brute-force loops on
// the host.
//
// The candidates of a call are the rows i with (cand_type == FILTER_ANY_TYPE or node_type[i] == cand_type) and (no pool or i
// listed in the pool), ascending by row index.  The pool arrives as an index list in any order, duplicates allowed: one
// launch sets bit i & 31 of word i >> 5 of a zeroed bitmap of filter_bitmap_words(n) words for every listed i (an atomic OR:
// order and duplicates vanish here, and the bitmap is the same whatever the launch's schedule).  The list is then compacted
// as cand_plan.h compacts a node type's: every workgroup counts the matches among its CAND_BLOCK rows, cand_plan.h's
// one-workgroup scan turns the counts into exclusive offsets, every workgroup scatters its matches to offset[block] +
// (matches before the row inside the block).  A row's position depends on the bitmap and the node types of the rows before
// it only, so the list is ascending, free of duplicates and the same on every run.  filter_block_offsets() is the offset
// table as the first launches leave it, filter_list() the list the scatter leaves.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "cand_plan.h"
#include "eval_plan.h"
#include "exclude_plan.h"

namespace rwr {

// ---- geometry of the list build --------------------------------------------------------------------------------------------
constexpr int32_t FILTER_ANY_TYPE = -1;           // cand_type: nodes of every type
constexpr int32_t FILTER_MARK_BLOCK = 256;        // threads per workgroup of the marking launch, one pool entry per thread and trip
constexpr int64_t FILTER_MARK_BLOCKS_MAX = 4096;  // its workgroups at most: a longer pool takes further trips (grid stride)

constexpr size_t filter_bitmap_words(int32_t n) { return n > 0 ? ((size_t)n + 31) / 32 : 0; }
constexpr size_t filter_word(int32_t i) { return (size_t)i >> 5; }
constexpr uint32_t filter_bit(int32_t i) { return 1u << (i & 31); }
constexpr int32_t filter_mark_blocks(int64_t pool_count)
{
    return pool_count <= 0 ? 0
                           : (int32_t)((pool_count + FILTER_MARK_BLOCK - 1) / FILTER_MARK_BLOCK < FILTER_MARK_BLOCKS_MAX
                                           ? (pool_count + FILTER_MARK_BLOCK - 1) / FILTER_MARK_BLOCK
                                           : FILTER_MARK_BLOCKS_MAX);
}

// is row i a candidate; bitmap == nullptr: no pool, every bit counts as set
constexpr bool filter_match(const uint8_t *node_type, int32_t cand_type, const uint32_t *bitmap, int32_t i)
{
    return (cand_type == FILTER_ANY_TYPE || node_type[i] == cand_type) && (!bitmap || (bitmap[filter_word(i)] & filter_bit(i)) != 0);
}

// the bitmap as the marking launch leaves it (entries outside [0, n) never reach it: filter_check refuses them)
inline std::vector<uint32_t> filter_bitmap(int32_t n, int64_t pool_count, const int32_t *pool_idx)
{
    std::vector<uint32_t> bm(filter_bitmap_words(n), 0u);
    for (int64_t q = 0; q < pool_count; ++q)
        if (pool_idx[q] >= 0 && pool_idx[q] < n) bm[filter_word(pool_idx[q])] |= filter_bit(pool_idx[q]);
    return bm;
}

// off[b] = candidates below block b, off[cand_blocks(n)] = length of the list: per-block counts, then the chunked exclusive
// scan with its carry, as the kernels run them (cand_block_offsets with filter_match for the type test)
inline std::vector<int32_t> filter_block_offsets(const uint8_t *node_type, int32_t n, int32_t cand_type, const uint32_t *bitmap)
{
    const int32_t nb = cand_blocks(n);
    std::vector<int32_t> off((size_t)nb + 1, 0);
    for (int32_t b = 0; b < nb; ++b)
        for (int32_t i = cand_block_lo(b); i < cand_block_hi(b, n); ++i) off[b] += filter_match(node_type, cand_type, bitmap, i);
    int32_t carry = 0;
    for (int32_t c0 = 0; c0 < nb; c0 += CAND_SCAN_CHUNK) {
        const int32_t c1 = nb - c0 < CAND_SCAN_CHUNK ? nb : c0 + CAND_SCAN_CHUNK;
        for (int32_t b = c0; b < c1; ++b) {
            const int32_t cnt = off[b];
            off[b] = carry;
            carry += cnt;
        }
    }
    off[nb] = carry;
    return off;
}

// the list as the scatter leaves it: block b's matches from off[b] on, in row order
inline std::vector<int32_t> filter_list(const uint8_t *node_type, int32_t n, int32_t cand_type, const uint32_t *bitmap,
                                        const std::vector<int32_t> &off)
{
    const int32_t nb = cand_blocks(n);
    std::vector<int32_t> rows((size_t)off[(size_t)nb], -1);
    for (int32_t b = 0; b < nb; ++b) {
        int32_t pos = off[(size_t)b];
        for (int32_t i = cand_block_lo(b); i < cand_block_hi(b, n); ++i)
            if (filter_match(node_type, cand_type, bitmap, i)) rows[(size_t)pos++] = i;
    }
    return rows;
}

// ---- the arguments of the two filtered entries ------------------------------------------------------------------------------
enum FilterVerdict : int32_t {
    FILTER_OK = 0,
    FILTER_NOOP = 1,          // K == 0 with a graph: nothing to do, RWR_OK
    FILTER_TYPED = 2,         // typed.verdict says what: the graph, K, the pointers, top_n < 1, cand_type, the mask, a seed
    FILTER_NULL_POOL = 3,     // pool_count > 0 with a NULL pool_idx                       (RWR_E_INVALID)
    FILTER_POOL_RANGE = 4,    // pool_idx[bad_pos] = bad_index is outside [0, n)           (RWR_E_RANGE)
    FILTER_DENY = 5,          // deny.verdict says what (exclude_check over the deny lists)
    FILTER_TEST = 6,          // test.verdict says what (eval_check; the positions entry only)
    FILTER_TOP_N_LIMIT = 7,   // top_n > top_n_max: the select path's limit                (RWR_E_UNSUPPORTED)
};

struct FilterCheck {
    FilterVerdict verdict = FILTER_OK;
    TypedCheck typed;         // cand_type FILTER_ANY_TYPE is legal here: BAD_CAND_TYPE means outside [-1, 255]
    int64_t bad_pos = -1;     // POOL_RANGE: the first offending position of the pool ...
    int32_t bad_index = 0;    // ... and the index found there
    ExcludeCheck deny;
    EvalCheck test;
};

// The pool and the deny lists, in this order: the pool's pointer, its first index out of range, then exclude_check's order
// over the deny lists (deny_ptr == nullptr: none).  pool_count < 0: no pool, pool_idx is not read.
inline void filter_sets_check(FilterCheck &c, int32_t n, int32_t K, int64_t pool_count, const int32_t *pool_idx,
                              const int64_t *deny_ptr, const int32_t *deny_idx)
{
    if (pool_count > 0 && !pool_idx) { c.verdict = FILTER_NULL_POOL; return; }
    for (int64_t q = 0; q < pool_count; ++q)
        if (pool_idx[q] < 0 || pool_idx[q] >= n) {
            c.verdict = FILTER_POOL_RANGE; c.bad_pos = q; c.bad_index = pool_idx[q];
            return;
        }
    if (deny_ptr) {
        c.deny = exclude_check(n, K, deny_ptr, deny_idx);
        if (c.deny.verdict != EXCLUDE_OK) c.verdict = FILTER_DENY;
    }
}

// rwr_recommend_filtered_batch.  In this order: what typed_check reports for the graph, K, the pointers, top_n's lower bound,
// the candidate type (now [-1, 255]), the mask and every seed; the pool; the deny lists; top_n's limit.
inline FilterCheck filter_check(bool have_graph, int32_t n, const int32_t *seeds, int32_t K, int32_t top_n, int32_t top_n_max,
                                int32_t cand_type, uint32_t excl_edge_mask, bool have_outputs, int64_t pool_count,
                                const int32_t *pool_idx, const int64_t *deny_ptr, const int32_t *deny_idx)
{
    FilterCheck c;
    c.typed = typed_check(have_graph, n, seeds, K, top_n, 0x7FFFFFFF, cand_type == FILTER_ANY_TYPE ? 0 : cand_type, excl_edge_mask,
                          have_outputs);
    if (c.typed.verdict == TYPED_NOOP) { c.verdict = FILTER_NOOP; return c; }
    if (c.typed.verdict != TYPED_OK) { c.verdict = FILTER_TYPED; return c; }
    filter_sets_check(c, n, K, pool_count, pool_idx, deny_ptr, deny_idx);
    if (c.verdict != FILTER_OK) return c;
    if (top_n > top_n_max) c.verdict = FILTER_TOP_N_LIMIT;
    return c;
}

// rwr_recommend_filtered_positions_batch: there is no top_n; NULL_ARG means NULL seeds; after the deny lists eval_check's
// verdict on the test sets, pos_out standing where the evaluating entries have their result arrays.
inline FilterCheck filter_positions_check(bool have_graph, int32_t n, const int32_t *seeds, int32_t K, int32_t cand_type,
                                          uint32_t excl_edge_mask, int64_t pool_count, const int32_t *pool_idx,
                                          const int64_t *deny_ptr, const int32_t *deny_idx, const int64_t *test_ptr,
                                          const int64_t *test_ids, const void *pos_out)
{
    FilterCheck c;
    c.typed = typed_check(have_graph, n, seeds, K, 1, 1, cand_type == FILTER_ANY_TYPE ? 0 : cand_type, excl_edge_mask, true);
    if (c.typed.verdict == TYPED_NOOP) { c.verdict = FILTER_NOOP; return c; }
    if (c.typed.verdict != TYPED_OK) { c.verdict = FILTER_TYPED; return c; }
    filter_sets_check(c, n, K, pool_count, pool_idx, deny_ptr, deny_idx);
    if (c.verdict != FILTER_OK) return c;
    c.test = eval_check(K, test_ptr, test_ids, pos_out, pos_out);
    if (c.test.verdict != EVAL_OK) c.verdict = FILTER_TEST;
    return c;
}

}  // namespace rwr
