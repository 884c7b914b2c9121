// What one rwr_recommend_filtered_batch / rwr_recommend_filtered_positions_batch call decides on the host about its candidates
// (DESIGN §3.20): the geometry of the device-side build of its candidate list from the caller's pool -- carried out by
// filter.hip -- and the host model of that build, which is the model of cand_plan.h's per-type lists as well (no pool).  (The
// verdict on the arguments is typed_call.h's.)  Plain C++17 without HIP, so that tests/cpp/filter_plan_check.cpp checks it
// against brute-force loops on the host.
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

// the bitmap as the marking launch leaves it (entries outside [0, n) never reach it: typed_call_check refuses them)
inline std::vector<uint32_t> filter_bitmap(int32_t n, int64_t pool_count, const int32_t *pool_idx)
{
    std::vector<uint32_t> bm(filter_bitmap_words(n), 0u);
    for (int64_t q = 0; q < pool_count; ++q)
        if (pool_idx[q] >= 0 && pool_idx[q] < n) bm[filter_word(pool_idx[q])] |= filter_bit(pool_idx[q]);
    return bm;
}

// off[b] = candidates below block b, off[cand_blocks(n)] = length of the list: per-block counts, then the chunked exclusive
// scan with its carry, as the kernels run them
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

}  // namespace rwr
