// What one rwr_recommend_typed_batch call decides on the host: the verdict on its arguments, which cached
// candidate list serves the call (or which entry is rebuilt), and the geometry of the device-side compaction that builds a
// list -- carried out by typed.hip.  Plain C++17 without HIP, so that tests/cpp/cand_plan_check.cpp checks all three against
// brute-force loops on the host.
//
// The candidate list of node type t is the rows with node_type == t, ascending by row index.  It is compacted in three
// launches: every workgroup counts the matches among its CAND_BLOCK consecutive rows (one row per thread); one workgroup
// turns the counts into exclusive offsets, CAND_SCAN_CHUNK counts per trip with a running carry; every workgroup then
// scatters its matches to offset[block] + (matches before the row inside the block).  A row's position depends on the
// rows before it only -- no atomic decides a position -- so the list is the same on every run.  cand_block_offsets() is
// that table as the first two launches leave it.
//
// Node types of resident nodes never change and nodes are only ever appended behind the last one (rwr_graph_append_nodes),
// so the list built while the graph had n nodes is valid exactly as long as the graph still has n nodes: that comparison is
// the cache's whole validity test, and no (re)build has to reset anything.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace rwr {

// ---- geometry of the compaction ------------------------------------------------------------------------------------------
constexpr int32_t CAND_BLOCK = 256;        // rows per workgroup = threads per workgroup
constexpr int32_t CAND_SCAN_CHUNK = 256;   // block counts the scanning workgroup takes per trip (one per thread)

constexpr int32_t cand_blocks(int32_t n) { return n > 0 ? (int32_t)(((int64_t)n + CAND_BLOCK - 1) / CAND_BLOCK) : 0; }
// rows [lo, hi) of block b
constexpr int32_t cand_block_lo(int32_t b) { return b * CAND_BLOCK; }
constexpr int32_t cand_block_hi(int32_t b, int32_t n) { return n - b * CAND_BLOCK < CAND_BLOCK ? n : (b + 1) * CAND_BLOCK; }

// off[b] = rows of type t below block b, off[cand_blocks(n)] = length of the list: per-block counts, then the chunked
// exclusive scan with its carry, as the kernels run them
inline std::vector<int32_t> cand_block_offsets(const uint8_t *node_type, int32_t n, int32_t t)
{
    const int32_t nb = cand_blocks(n);
    std::vector<int32_t> off((size_t)nb + 1, 0);
    for (int32_t b = 0; b < nb; ++b)
        for (int32_t i = cand_block_lo(b); i < cand_block_hi(b, n); ++i) off[b] += node_type[i] == t;
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

// ---- the cache of a handle ------------------------------------------------------------------------------------------------
constexpr int CAND_CACHE = 4;              // lists kept per handle (the header names four node types)

struct CandEntry {
    int32_t type = -1;                     // node type of the list, -1 = the entry is empty
    int32_t n = -1;                        // node count of the graph when the list was built
    int32_t rows = 0;                      // length of the list
    uint64_t used = 0;                     // the handle's call counter at the entry's last use
};

struct CandChoice {
    int entry = 0;
    bool hit = false;                      // the entry's list serves the call as it is; otherwise it is (re)built there
};

// The entry for node type `type` on a graph of n nodes.  An entry of that type: a hit when it was built for n nodes, else
// rebuilt in place.  No such entry: the first empty one, else the first whose list is stale (built for another n), else the
// one used longest ago (the lowest index among equals).
inline CandChoice cand_cache_choose(const CandEntry *e, int32_t type, int32_t n)
{
    for (int i = 0; i < CAND_CACHE; ++i)
        if (e[i].type == type) return {i, e[i].n == n};
    for (int i = 0; i < CAND_CACHE; ++i)
        if (e[i].type < 0) return {i, false};
    for (int i = 0; i < CAND_CACHE; ++i)
        if (e[i].n != n) return {i, false};
    int lru = 0;
    for (int i = 1; i < CAND_CACHE; ++i)
        if (e[i].used < e[lru].used) lru = i;
    return {lru, false};
}

// ---- the arguments of rwr_recommend_typed_batch -----------------------------------------------------------------------------
constexpr uint32_t TYPED_EDGE_TYPES = 8;   // edge types the header names: bit t of the mask stands for type t < 8

enum TypedVerdict : int32_t {
    TYPED_OK = 0,
    TYPED_NOOP = 1,           // K == 0: nothing to do, RWR_OK
    TYPED_NULL_GRAPH = 2,     // refused before anything else                  (RWR_E_INVALID)
    TYPED_NEGATIVE_K = 3,     //                                               (RWR_E_INVALID)
    TYPED_NULL_ARG = 4,       // NULL seeds, ids, scores or counts with K > 0  (RWR_E_INVALID)
    TYPED_BAD_TOP_N = 5,      // top_n < 1                                     (RWR_E_INVALID)
    TYPED_BAD_CAND_TYPE = 6,  // cand_type outside [0, 255]                    (RWR_E_INVALID)
    TYPED_BAD_MASK = 7,       // a mask bit >= TYPED_EDGE_TYPES                (RWR_E_INVALID)
    TYPED_SEED_RANGE = 8,     // seeds[bad_k] = bad_seed is outside [0, n)     (RWR_E_RANGE)
    TYPED_TOP_N_LIMIT = 9,    // top_n > top_n_max: the select path's limit    (RWR_E_UNSUPPORTED)
};

struct TypedCheck {
    TypedVerdict verdict = TYPED_OK;
    int32_t bad_k = -1;       // SEED_RANGE: the first offending batch position ...
    int32_t bad_seed = 0;     // ... and the seed found there
};

// In this order: the graph, K, the pointers, top_n's lower bound, the candidate type, the mask, every seed, top_n's limit.
// n: the graph's node count (not read without a graph).
inline TypedCheck typed_check(bool have_graph, int32_t n, const int32_t *seeds, int32_t K, int32_t top_n, int32_t top_n_max,
                              int32_t cand_type, uint32_t excl_edge_mask, bool have_outputs)
{
    TypedCheck c;
    if (!have_graph) { c.verdict = TYPED_NULL_GRAPH; return c; }
    if (K < 0) { c.verdict = TYPED_NEGATIVE_K; return c; }
    if (K == 0) { c.verdict = TYPED_NOOP; return c; }
    if (!seeds || !have_outputs) { c.verdict = TYPED_NULL_ARG; return c; }
    if (top_n < 1) { c.verdict = TYPED_BAD_TOP_N; return c; }
    if (cand_type < 0 || cand_type > 255) { c.verdict = TYPED_BAD_CAND_TYPE; return c; }
    if (excl_edge_mask >> TYPED_EDGE_TYPES) { c.verdict = TYPED_BAD_MASK; return c; }
    for (int32_t k = 0; k < K; ++k)
        if (seeds[k] < 0 || seeds[k] >= n) {
            c.verdict = TYPED_SEED_RANGE; c.bad_k = k; c.bad_seed = seeds[k];
            return c;
        }
    if (top_n > top_n_max) { c.verdict = TYPED_TOP_N_LIMIT; return c; }
    return c;
}

}  // namespace rwr
