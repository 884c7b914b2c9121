// Which nodes and links of one rwr_graph_remove_nodes call leave a resident graph and where everything else goes (DESIGN
// §3.24), decided by node_remove_plan() from the handle's host state and the call's node list alone and carried out by
// graph_remove_nodes (node_remove.hip).  Plain C++17 without HIP types, so that tests/cpp/node_remove_plan_check.cpp checks it
// against a list-of-lists erase on the host; what the device kernels compute per link, per chunk and per lane (nrm_* below) is
// __host__ __device__ and runs in that program as well.
//
// Nodes.  The surviving nodes close up and keep their order: old node i becomes new_index[i] = i - #{removed nodes < i}, a
// strictly increasing function of the survivors onto [0, n_new).
//
// Links.  A link leaves if its source or its target is a removed node.  The host knows the sources: the links of a removed
// row i are the old flat positions [rowptr[i], rowptr[i + 1]), and the removed rows give sorted, disjoint, non-empty intervals
// (consecutive removed rows merge, empty rows give none).  The targets are known on the device only, so
//     keep(e) = e lies in no removed interval && !removed(dst[e])
// is evaluated there, per link.  Everything else keeps its order, so the kept old position e moves to
//     new position = #{kept e' < e}
// which is strictly increasing over the kept positions and takes every value of [0, m_new) once.  The device forms it as
// offset[chunk] + (kept positions of the chunk in front of e): an exclusive scan of the chunks' kept counts, plus a rank inside
// the chunk from wave ballots -- sums of counts only, so no atomic decides a position.  A row pointer is a position too:
// rowptr_new[new_index[i]] = #{kept e' < rowptr[i]} for every surviving row i, and rowptr_new[n_new] = m_new.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define NRM_HD __host__ __device__
#else
#define NRM_HD
#endif

namespace rwr {

// ---- what the device kernels compute (node_remove.hip)
constexpr int NRM_CHUNK = 8192;     // old link positions per workgroup (§3.23's geometry)
constexpr int NRM_THREADS = 256;
constexpr int NRM_WAVE = 64;
constexpr int NRM_WAVES = NRM_THREADS / NRM_WAVE;
constexpr int NRM_TRIPS = NRM_CHUNK / NRM_THREADS;

// chunks of a list of m_old links: at least one, so that a graph without links still has a workgroup for its row pointers
NRM_HD inline int64_t nrm_chunks(int64_t m_old) { return m_old > 0 ? (m_old + NRM_CHUNK - 1) / NRM_CHUNK : 1; }

// bit i of the removed-node bitmap ((n + 7) / 8 bytes)
NRM_HD inline bool nrm_removed(const uint8_t *bits, int32_t i) { return (bits[i >> 3] >> (i & 7)) & 1; }

// first k in [lo, hi) with a[k] >= v (hi if there is none); a non-decreasing
NRM_HD inline int64_t nrm_lower_bound(const int64_t *a, int64_t lo, int64_t hi, int64_t v)
{
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
// first k in [lo, hi) with a[k] > v
NRM_HD inline int64_t nrm_upper_bound(const int64_t *a, int64_t lo, int64_t hi, int64_t v)
{
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] <= v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// The removed intervals [iv_lo[k], iv_hi[k]) that meet the chunk [c0, c1) of old positions: k in [j, jend).  The intervals are
// sorted and disjoint, so both iv_lo and iv_hi ascend strictly: the ones in front of the chunk end at or before c0, the ones
// behind it start at or after c1.
struct NrmSlice { int64_t j, jend; };
NRM_HD inline NrmSlice nrm_chunk_slice(const int64_t *iv_lo, const int64_t *iv_hi, int64_t ni, int64_t c0, int64_t c1)
{
    NrmSlice s;
    s.j = nrm_upper_bound(iv_hi, 0, ni, c0);         // first interval with hi > c0
    s.jend = nrm_lower_bound(iv_lo, s.j, ni, c1);    // first interval with lo >= c1
    return s;
}

// does old position e of the chunk lie in a removed interval (the chunk's own slice decides: see above)
NRM_HD inline bool nrm_in_removed_row(const int64_t *iv_lo, const int64_t *iv_hi, NrmSlice s, int64_t e)
{
    const int64_t k = nrm_upper_bound(iv_hi, s.j, s.jend, e);   // first interval of the slice with hi > e
    return k < s.jend && iv_lo[k] <= e;
}

// THE keep predicate of the link at old position e with target dst_e.  (Every resident target lies in [0, n): the build
// refuses anything else.  The comparison only keeps a damaged array from indexing the bitmap outside its bytes.)
NRM_HD inline bool nrm_keep(const int64_t *iv_lo, const int64_t *iv_hi, NrmSlice s, const uint8_t *bits, int32_t n, int64_t e,
                            int32_t dst_e)
{
    return !nrm_in_removed_row(iv_lo, iv_hi, s, e) && (uint32_t)dst_e < (uint32_t)n && !nrm_removed(bits, dst_e);
}

// kept elements of a wave in front of lane `lane`, from the wave's ballot of the keep predicate
NRM_HD inline int nrm_lane_rank(unsigned long long ballot, int lane)
{
    const unsigned long long below = ballot & ((1ull << lane) - 1ull);
#if defined(__HIP_DEVICE_COMPILE__)
    return __popcll(below);
#else
    return __builtin_popcountll(below);
#endif
}
NRM_HD inline int nrm_wave_count(unsigned long long ballot)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __popcll(ballot);
#else
    return __builtin_popcountll(ballot);
#endif
}

// Kept positions of the chunk in front of the element that lane `lane` of wave `wv` takes in one trip: `base` = the kept
// elements of the earlier trips, wc[q] = those of wave q in this trip.  Trips, waves and lanes walk the chunk in position
// order (element = c0 + trip * NRM_THREADS + wv * NRM_WAVE + lane), so this is the element's exclusive prefix in the chunk.
NRM_HD inline int nrm_rank_in_chunk(int base, const int *wc, int wv, unsigned long long ballot, int lane)
{
    int r = base;
    for (int q = 0; q < wv; ++q) r += wc[q];
    return r + nrm_lane_rank(ballot, lane);
}

// The row starts a chunk's workgroup writes: the entries i of rowptr_old[0 .. n] (the end n included: "row" n with new index
// n_new) whose value falls into [c0, c1) -- and, for the LAST chunk, the ones equal to m_old as well, which no chunk contains
// (trailing rows without links, and the end).  Empty rows share a start with their successor and are all inside the range.
struct NrmRows { int64_t lo, hi; };
NRM_HD inline NrmRows nrm_chunk_rows(const int64_t *rowptr_old, int32_t n, int64_t c0, int64_t c1, bool last_chunk)
{
    NrmRows r;
    r.lo = nrm_lower_bound(rowptr_old, 0, (int64_t)n + 1, c0);
    r.hi = last_chunk ? (int64_t)n + 1 : nrm_lower_bound(rowptr_old, r.lo, (int64_t)n + 1, c1);
    return r;
}

// ---- compaction of a list of rows (item_rows, item_order): entry q stays if its row does, and carries the row's new index.
// Geometry: CAND_BLOCK-style blocks of NRM_THREADS entries, one per thread; offsets by launch_cand_scan (int32 suffices).
NRM_HD inline int32_t nrm_list_blocks(int32_t len) { return len > 0 ? (len + NRM_THREADS - 1) / NRM_THREADS : 0; }

// ---- the host plan
enum NodeRemoveVerdict : int32_t {
    NODE_REMOVE_OK = 0,
    NODE_REMOVE_BAD_RANGE = 1,    // node_index[bad_q] outside [0, n)
    NODE_REMOVE_DUPLICATE = 2,    // node_index[bad_q] equals an earlier entry (bad_q is the second occurrence)
    NODE_REMOVE_ALL = 3,          // count == n: a graph cannot lose its last node
};

struct NodeRemovePlan {
    NodeRemoveVerdict verdict = NODE_REMOVE_OK;
    int32_t bad_q = -1;
    int32_t n_old = 0, n_new = 0;
    int64_t m_old = 0;
    int64_t m_rows = 0;                  // links of the removed rows: m_new <= m_old - m_rows, with equality iff no kept row
                                         // links to a removed node (the device finds that out)
    std::vector<uint8_t> bits;           // [(n_old + 7) / 8] removed-node bitmap
    std::vector<int32_t> new_index;      // [n_old + 1] new index of old node i, -1 = removed; [n_old] = n_new
    std::vector<int64_t> iv_lo, iv_hi;   // the removed rows' link intervals: sorted, disjoint, non-empty
    std::vector<uint8_t> is_item_new;    // [n_new] h_is_item compacted
    int32_t n_items_new = 0;
};

// rowptr: the n + 1 host row pointers; is_item: the n host ITEM flags.  Validation looks at every entry before anything is
// planned, through a byte map over n (not a sort: the duplicate verdict names the SECOND occurrence, i.e. the first q whose
// node is already marked): the first index out of range, else the first repeat, else count == n.
inline NodeRemovePlan node_remove_plan(int32_t n, const int64_t *rowptr, const uint8_t *is_item, int32_t count,
                                       const int32_t *node_index)
{
    NodeRemovePlan p;
    p.n_old = p.n_new = n;
    p.m_old = rowptr[n];
    if (count < 0) count = 0;
    for (int32_t q = 0; q < count; ++q)
        if (node_index[q] < 0 || node_index[q] >= n) { p.verdict = NODE_REMOVE_BAD_RANGE; p.bad_q = q; return p; }
    std::vector<uint8_t> mark((size_t)n, 0);
    for (int32_t q = 0; q < count; ++q) {
        uint8_t &mk = mark[(size_t)node_index[q]];
        if (mk) { p.verdict = NODE_REMOVE_DUPLICATE; p.bad_q = q; return p; }
        mk = 1;
    }
    if (count == n) { p.verdict = NODE_REMOVE_ALL; return p; }

    p.n_new = n - count;
    p.bits.assign(((size_t)n + 7) / 8, 0);
    p.new_index.resize((size_t)n + 1);
    p.is_item_new.resize((size_t)p.n_new);
    int32_t at = 0;
    for (int32_t i = 0; i < n; ++i) {               // the one O(n) walk
        if (mark[(size_t)i]) {
            p.bits[(size_t)(i >> 3)] |= (uint8_t)(1u << (i & 7));
            p.new_index[(size_t)i] = -1;
            const int64_t a = rowptr[i], b = rowptr[(size_t)i + 1];
            if (b > a) {
                p.m_rows += b - a;
                if (!p.iv_hi.empty() && p.iv_hi.back() == a) p.iv_hi.back() = b;   // (the row before it was removed too,
                else { p.iv_lo.push_back(a); p.iv_hi.push_back(b); }              //  or only empty rows lie in between)
            }
        } else {
            p.new_index[(size_t)i] = at;
            p.is_item_new[(size_t)at] = is_item[i];
            p.n_items_new += is_item[i] ? 1 : 0;
            ++at;
        }
    }
    p.new_index[(size_t)n] = p.n_new;
    return p;
}

}  // namespace rwr
