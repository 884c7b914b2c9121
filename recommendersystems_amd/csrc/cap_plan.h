// What one rwr_recommend_capped_batch / rwr_recommend_capped_positions_batch call decides on the host about its cap (DESIGN
// §3.21): the sort key of a labelled candidate, the geometry of the segments and chunks the device-side selection works on,
// and a host model of that selection -- carried out by group_cap.hip.  (The verdict on the arguments is typed_call.h's.)
// Plain C++17 without HIP (the few functions the kernels share carry CAP_HD), so that tests/cpp/cap_plan_check.cpp checks all
// of it against brute-force loops on the host.
//
// The cap keeps, per seed, at most m = group_cap candidates of every group: a candidate stays iff fewer than m candidates of
// its label rank before it in that seed's list.  On the device that is a per-group, per-column top-m over the rank matrix:
//   1. the rows of the call's ascending candidate list whose label is >= 0 become keys cap_key(label, row); sorted, the keys
//      of one label are contiguous (a SEGMENT) with the rows ascending inside it, whatever the launches' schedule;
//   2. a segment of at most m rows can lose nobody and is left out of the plan; a longer one is cut into CHUNKS of at most
//      `chunk` rows (CAP_CHUNK unless a test selects a smaller one); one wave serves one (chunk, tile);
//   3. the wave keeps, per column, the CAP_MAX-slot list CapList of the best keys it has seen -- cap_rank_key(score, id, row):
//      the rankers' order (score descending, id descending) with the smaller row winning among equal pairs; the list's last
//      slot is the m-th best key, the column's THRESHOLD;
//   4. a segment of one chunk is finished by the same wave: every live cell of the chunk whose key is worse than the
//      threshold receives -1.  A segment of several chunks has its chunks' lists merged per column (cap_list_merge) into
//      the segment's threshold first, and its chunks are marked in a launch of their own.
// cap_threshold() is steps 3-4's threshold as the kernels compute it; cap_plan() the tables of step 2.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "filter_plan.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CAP_HD __host__ __device__ __forceinline__
#else
#define CAP_HD inline
#endif

namespace rwr {

// ---- the sort key of a labelled candidate ------------------------------------------------------------------------------------
constexpr int32_t CAP_MAX = 8;          // == RWR_GROUP_CAP_MAX (group_cap.hip asserts it): slots of a column's list, in registers
constexpr int32_t CAP_CHUNK = 512;      // rows of a chunk at most: a wave's share of a long segment

CAP_HD uint64_t cap_key(int32_t label, int32_t row) { return (uint64_t)(uint32_t)label << 32 | (uint64_t)(uint32_t)row; }
CAP_HD int32_t cap_key_label(uint64_t key) { return (int32_t)(uint32_t)(key >> 32); }
CAP_HD int32_t cap_key_row(uint64_t key) { return (int32_t)(uint32_t)key; }
// bits of the keys of labels in [0, max_label]: the row's 32 and the label's (at least one: the sort takes no shorter key)
inline int cap_key_bits(int32_t max_label)
{
    int b = 0;
    for (uint32_t v = max_label > 0 ? (uint32_t)max_label : 0u; v; v >>= 1) ++b;
    return 32 + (b > 0 ? b : 1);
}

// the sorted keys of a candidate list (ascending, duplicate-free rows): what the compaction and the sort leave.  The
// compaction keeps the list's order, so a stable sort by label alone is the sort by key
inline std::vector<uint64_t> cap_sorted_keys(const int32_t *rows, int32_t nrows, const int32_t *group_of)
{
    std::vector<uint64_t> keys;
    for (int32_t p = 0; p < nrows; ++p)
        if (group_of[rows[p]] >= 0) keys.push_back(cap_key(group_of[rows[p]], rows[p]));
    for (size_t i = 1; i < keys.size(); ++i) {                  // (insertion sort: the model is for small inputs)
        const uint64_t k = keys[i];
        size_t j = i;
        for (; j > 0 && keys[j - 1] > k; --j) keys[j] = keys[j - 1];
        keys[j] = k;
    }
    return keys;
}

// is position p of the sorted keys the head of a segment
CAP_HD bool cap_is_head(const uint64_t *keys, int32_t p) { return p == 0 || (keys[p] >> 32) != (keys[p - 1] >> 32); }

// the head positions, ascending, and the list's length behind them: segment s is positions [start[s], start[s + 1])
inline std::vector<int32_t> cap_segment_starts(const std::vector<uint64_t> &keys)
{
    std::vector<int32_t> start;
    for (int32_t p = 0; p < (int32_t)keys.size(); ++p)
        if (cap_is_head(keys.data(), p)) start.push_back(p);
    start.push_back((int32_t)keys.size());
    return start;
}

// ---- segments and chunks --------------------------------------------------------------------------------------------------------
// Planned segments are the segments longer than m, numbered in the order of the sorted list; chunks are numbered segment by
// segment, a segment's chunks in position order.  `single` lists the chunks of one-chunk segments (the fused launch's
// work), `multi` the chunks of the others in the same order (the split launches' work, a segment's chunks adjacent);
// multi-chunk segment j owns multi[mseg_first[j] .. + mseg_count[j]), and multi_mseg[i] = the j of multi[i].
struct CapPlan {
    std::vector<int32_t> chunk_pos, chunk_len, chunk_seg;       // chunk -> first position, length, planned segment
    std::vector<int32_t> seg_pos, seg_len, seg_chunk0, seg_nchunks;   // planned segment -> its run, first chunk, chunk count
    std::vector<int32_t> single, multi, multi_mseg, mseg_first, mseg_count;
};

constexpr int32_t cap_chunks_of(int32_t len, int32_t chunk) { return (int32_t)(((int64_t)len + chunk - 1) / chunk); }

// start: nseg + 1 ascending positions (cap_segment_starts); m in [1, CAP_MAX]; chunk >= 1
inline CapPlan cap_plan(const int32_t *start, int32_t nseg, int32_t m, int32_t chunk)
{
    CapPlan pl;
    for (int32_t s = 0; s < nseg; ++s) {
        const int32_t pos = start[s], len = start[s + 1] - start[s];
        if (len <= m) continue;                                  // nobody can be dropped: no work
        const int32_t seg = (int32_t)pl.seg_pos.size(), nc = cap_chunks_of(len, chunk);
        pl.seg_pos.push_back(pos), pl.seg_len.push_back(len);
        pl.seg_chunk0.push_back((int32_t)pl.chunk_pos.size()), pl.seg_nchunks.push_back(nc);
        if (nc > 1) pl.mseg_first.push_back((int32_t)pl.multi.size()), pl.mseg_count.push_back(nc);
        for (int32_t c = 0; c < nc; ++c) {
            const int32_t id = (int32_t)pl.chunk_pos.size();
            pl.chunk_pos.push_back(pos + c * chunk);
            pl.chunk_len.push_back(len - c * chunk < chunk ? len - c * chunk : chunk);
            pl.chunk_seg.push_back(seg);
            if (nc == 1) pl.single.push_back(id);
            else pl.multi.push_back(id), pl.multi_mseg.push_back((int32_t)pl.mseg_first.size() - 1);
        }
    }
    return pl;
}

// ---- the selection: a column's best m keys ---------------------------------------------------------------------------------------
// hi = the score's order-preserving bits (>= 2^63: live scores are >= +0.0), lo = the id's, rw = 0x7FFFFFFF - row: the larger
// key ranks first.  {0, 0, 0} lies below every real key, {~0, ~0, ~0} above
struct CapKey {
    uint64_t hi, lo;
    uint32_t rw;
};

CAP_HD uint64_t cap_score_bits(double x)                        // (common.h's f64_orderable: -0.0 counts as +0.0)
{
    x = x + 0.0;
    uint64_t u;
    __builtin_memcpy(&u, &x, 8);
    return (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
}
CAP_HD CapKey cap_rank_key(double score, int64_t id, int32_t row)
{
    return CapKey{cap_score_bits(score), (uint64_t)id ^ 0x8000000000000000ull, 0x7FFFFFFFu - (uint32_t)row};
}
CAP_HD bool cap_better(const CapKey &a, const CapKey &b)
{
    return a.hi != b.hi ? a.hi > b.hi : a.lo != b.lo ? a.lo > b.lo : a.rw > b.rw;
}
CAP_HD bool cap_is_top(const CapKey &a) { return a.hi == ~0ull; }   // (no score has these bits: NaNs are not live)

// A column's list: slots [CAP_MAX - m, CAP_MAX) hold the best m keys seen, descending, {0, 0, 0} where fewer were seen; the
// slots in front of them hold the top sentinel, which nothing passes -- so the m-th best key is always the LAST slot and
// no slot is ever addressed by a run-time index (the list lives in registers).
struct CapList {
    CapKey k[CAP_MAX];
};
CAP_HD void cap_list_init(CapList &l, int32_t m)
{
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < CAP_MAX; ++j) l.k[j] = j < CAP_MAX - m ? CapKey{~0ull, ~0ull, ~0u} : CapKey{0, 0, 0};
}
CAP_HD const CapKey &cap_list_threshold(const CapList &l) { return l.k[CAP_MAX - 1]; }
// a key that beats the threshold takes the last slot and rises past every worse key
CAP_HD void cap_list_insert(CapList &l, const CapKey &key)
{
    if (!cap_better(key, l.k[CAP_MAX - 1])) return;
    l.k[CAP_MAX - 1] = key;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = CAP_MAX - 1; j > 0; --j)
        if (cap_better(l.k[j], l.k[j - 1])) {
            const CapKey t = l.k[j];
            l.k[j] = l.k[j - 1];
            l.k[j - 1] = t;
        }
}
// the real keys of another list of the same column (other rows) join this one
CAP_HD void cap_list_merge(CapList &l, const CapList &other)
{
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < CAP_MAX; ++j)
        if (!cap_is_top(other.k[j])) cap_list_insert(l, other.k[j]);
}

// The threshold of one column over positions [pos, pos + len) of the sorted keys, as the kernels compute it: col[row * stride]
// is the column's cell of that row (live: >= 0), node_id the ids; cut into chunks of `chunk` rows whose lists are merged in
// chunk order.  A live cell of the run is kept iff its key is not worse than the result.
inline CapKey cap_threshold(const double *col, size_t stride, const int64_t *node_id, const uint64_t *keys, int32_t pos, int32_t len,
                            int32_t m, int32_t chunk)
{
    CapList seg;
    cap_list_init(seg, m);
    for (int32_t c0 = 0; c0 < len; c0 += chunk) {
        CapList l;
        cap_list_init(l, m);
        for (int32_t p = pos + c0; p < pos + len && p < pos + c0 + chunk; ++p) {
            const int32_t row = cap_key_row(keys[p]);
            const double x = col[(size_t)row * stride];
            if (x >= 0.0) cap_list_insert(l, cap_rank_key(x, node_id[row], row));
        }
        cap_list_merge(seg, l);
    }
    return cap_list_threshold(seg);
}

}  // namespace rwr
