// What one rwr_recommend_typed_batch call decides on the host about its candidates: which cached candidate
// list serves the call (or which entry is rebuilt), and the geometry of the device-side compaction that builds a list --
// carried out by typed.hip.  (The verdict on the arguments is typed_call.h's.)  Plain C++17 without HIP, so that
// tests/cpp/cand_plan_check.cpp checks both against brute-force loops on the host.
//
// The candidate list of node type t is the rows with node_type == t, ascending by row index.  It is compacted in three
// launches: every workgroup counts the matches among its CAND_BLOCK consecutive rows (one row per thread); one workgroup
// turns the counts into exclusive offsets, CAND_SCAN_CHUNK counts per trip with a running carry; every workgroup then
// scatters its matches to offset[block] + (matches before the row inside the block).  A row's position depends on the
// rows before it only -- no atomic decides a position -- so the list is the same on every run.  The host model of the
// offset table and of the list is filter_plan.h's (filter_block_offsets, filter_list): a call's pool only narrows the match.
//
// Node types of resident nodes never change, and between two removals nodes are only ever appended behind the last one
// (rwr_graph_append_nodes), so the list built while the graph had n nodes is valid exactly as long as the graph still has n
// nodes: that comparison is the cache's whole validity test, and no (re)build has to reset anything.  The one edit that breaks
// the premise, rwr_graph_remove_nodes (after it a later append can bring n back to a cached value over other rows), empties
// every entry itself (node_remove.hip); cand_cache_choose never sees a list of another node set.
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

// ---- the edge-type mask of the typed entries -----------------------------------------------------------------------------------------
constexpr uint32_t TYPED_EDGE_TYPES = 8;   // edge types the header names: bit t of the mask stands for type t < 8

}  // namespace rwr
