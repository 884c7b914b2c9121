// The host plan of the long-list destination of the ranked end (rwr_recommend_long_batch, rwr_recommend_audience_set_long_batch,
// long_list.hip): lists of top_n in (LONG_SEL_MAX_K, LONG_TOP_N_MAX] entries.  Here: what the two entries add to
// their ladders (typed_call.h, audience_set_plan.h: only the top_n limit differs), the collect capacity of a segment, the run
// and pass tables of its sort, the buffer that holds the result, the merge-path partition -- the functions the kernels call as
// they stand -- the tile-by-tile split of a group whose buffers would be large, and a host model of the whole selection.
// Plain C++17 without HIP, so that tests/cpp/long_plan_check.cpp checks all of it on the host.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/rwr.h"
#include "audience_set_plan.h"
#include "typed_call.h"

#ifdef __HIPCC__
#define RWR_LONG_HD __host__ __device__
#else
#define RWR_LONG_HD
#endif

namespace rwr {

constexpr int32_t LONG_TOP_N_MAX = RWR_LONG_TOP_N_MAX;
constexpr int32_t LONG_SEL_MAX_K = 1024, LONG_SEL_CAP = 3072, LONG_SEL_LEVELS = 16;   // rank_keys.h: SEL_MAX_K, SEL_CAP, SEL_LEVELS
constexpr int32_t LONG_RUN = 4096;                // R: entries one workgroup sorts in LDS (4 096 x 24 B = 96 KiB)
constexpr int32_t LONG_MERGE_ITEMS = 8;           // outputs of one thread of a merge pass; divides 2 * LONG_RUN
constexpr int32_t LONG_NO_TIE = 0x7FFFFFFF;       // a segment's list-position threshold when its bin is taken whole
constexpr uint64_t LONG_WS_BYTES = 1ull << 30;    // both buffers of one pass over a group's tiles stay below this, or one tile's

// ---- the entries ---------------------------------------------------------------------------------------------------------------
// does a list of top_n entries go through the long destination (below: the stock select, launch for launch)
inline bool long_applies(int32_t top_n) { return top_n > LONG_SEL_MAX_K; }

// rwr_recommend_long_batch: rwr_recommend_explained_batch's description without reasons, the ladder's top_n limit replaced
inline void long_call_fill(TypedCall &c)
{
    c.any_type = true;
    c.dest = CALL_LISTS;
    c.n_why = 0, c.why_src = nullptr, c.why_term = nullptr, c.why_total = nullptr;
    c.top_n_max = LONG_TOP_N_MAX;
    c.top_n_what = "the long lists' limit";
    c.top_n_hint = " (the positions entries answer for whole lists)";
}
// rwr_recommend_audience_set_long_batch: rwr_recommend_audience_set_batch's description, top_n up to the long limit
inline void long_aud_fill(AudCall &c)
{
    c.dest = AUD_LISTS;
    c.top_n_max = LONG_TOP_N_MAX;
}

// ---- capacity, runs, passes ----------------------------------------------------------------------------------------------------
// Entries a segment can collect: the top_n - 1 at most that lie above the threshold's bin, and a bin of LONG_SEL_CAP members at
// most -- a larger bin means the 128 key bits are spent, and then exactly k_rem of its members are taken (long_tie_position).
inline int64_t long_capacity(int32_t top_n) { return (int64_t)top_n - 1 + LONG_SEL_CAP; }
inline int32_t long_runs(int64_t collected) { return (int32_t)((collected + LONG_RUN - 1) / LONG_RUN); }
// merge passes that leave one run: ceil(log2(runs)).  The launches are planned from the capacity: a segment that collected
// less runs the same passes, which copy what has no partner
inline int32_t long_passes(int64_t collected)
{
    const int32_t runs = long_runs(collected);
    int32_t p = 0;
    while (((int64_t)1 << p) < runs) ++p;
    return p;
}
// the run width pass p (from 0) reads, and the buffer (0: the collect's, 1: the other) that holds the result after `passes`
RWR_LONG_HD inline int64_t long_pass_width(int32_t p) { return (int64_t)LONG_RUN << p; }
inline int32_t long_result_buffer(int32_t passes) { return passes & 1; }

// One pair of pass p: outputs [base, base + la + lb) of a segment of cnt entries are the merge of the run [base, base + la) with
// the run [base + la, base + la + lb); lb == 0: a run without a partner, copied.  o: any output position below cnt
struct LongPair {
    int64_t base, la, lb;
};
RWR_LONG_HD inline LongPair long_pair_of(int64_t o, int64_t width, int64_t cnt)
{
    LongPair r;
    r.base = o / (2 * width) * (2 * width);
    const int64_t left = cnt - r.base;
    r.la = left < width ? left : width;
    r.lb = left - r.la < width ? left - r.la : width;
    return r;
}
struct LongPassRow {
    int64_t width, pairs, copied;   // pairs with a partner, runs copied
};
inline std::vector<LongPassRow> long_pass_table(int64_t collected)
{
    std::vector<LongPassRow> t;
    for (int32_t p = 0; p < long_passes(collected); ++p) {
        LongPassRow r{long_pass_width(p), 0, 0};
        for (int64_t o = 0; o < collected; o += 2 * r.width) (long_pair_of(o, r.width, collected).lb > 0 ? r.pairs : r.copied) += 1;
        t.push_back(r);
    }
    return t;
}

// ---- the order and the merge-path partition --------------------------------------------------------------------------------------
// rank_keys.h's SelCandRow, field for field: hi = f64_orderable(score), lo = i64_orderable(id); larger keys rank first, among
// equal (score, id) the smaller row -- a total order over distinct rows
struct LongKey {
    uint64_t hi, lo;
    int32_t row, pad;
};
RWR_LONG_HD inline bool long_key_lt(const LongKey &a, const LongKey &b)
{
    return a.hi != b.hi ? a.hi < b.hi : a.lo != b.lo ? a.lo < b.lo : a.row > b.row;
}
// How many of the first d outputs of the merge of A (la entries) and B (lb entries), both descending, come from A; an entry of
// A goes before an equal one of B.  0 <= d <= la + lb
RWR_LONG_HD inline int64_t long_merge_partition(const LongKey *A, int64_t la, const LongKey *B, int64_t lb, int64_t d)
{
    int64_t lo = d > lb ? d - lb : 0, hi = d < la ? d : la;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (!long_key_lt(A[mid], B[d - 1 - mid])) lo = mid + 1;   // A[mid] goes out before B[d - 1 - mid]: it is among the d
        else hi = mid;
    }
    return lo;
}
// outputs [d, d + count) of that merge into out
RWR_LONG_HD inline void long_merge_range(const LongKey *A, int64_t la, const LongKey *B, int64_t lb, int64_t d, int64_t count, LongKey *out)
{
    int64_t ai = long_merge_partition(A, la, B, lb, d), bi = d - ai;
    for (int64_t i = 0; i < count; ++i) {
        const bool from_a = bi >= lb || (ai < la && !long_key_lt(A[ai], B[bi]));
        out[i] = from_a ? A[ai++] : B[bi++];
    }
}

// ---- the tile-by-tile split ------------------------------------------------------------------------------------------------------
// bytes of the two entry buffers of `tiles` tiles of G segments, and the tiles of a group (tg > 0) one pass of the long end
// takes: as many as stay below LONG_WS_BYTES, one at least
inline uint64_t long_buffer_bytes(int64_t tiles, int G, int32_t top_n) { return 2ull * (uint64_t)tiles * (uint64_t)G * (uint64_t)long_capacity(top_n) * sizeof(LongKey); }
inline int32_t long_tiles_per_pass(int32_t tg, int G, int32_t top_n)
{
    const uint64_t one = long_buffer_bytes(1, G, top_n);
    const uint64_t fit = LONG_WS_BYTES / one;
    return (int32_t)(fit < 1 ? 1 : fit > (uint64_t)tg ? (uint64_t)tg : fit);
}

// ---- the host model of the selection ----------------------------------------------------------------------------------------------
// rank.hip's levels over the keys of one segment (its candidates in list order, the excluded ones left out): 8-bit digits of
// the 128-bit (hi, lo) from the top until the bin of the k-th best key holds LONG_SEL_CAP members at most or the bits are spent
struct LongThreshold {
    uint64_t ph = 0, pl = 0;
    int32_t nbits = 0, k_rem = 0;
    int64_t total = 0;
    int32_t q_tie = LONG_NO_TIE;      // nbits == 128: the list position of the k_rem-th member of the bin; the later ones are left out
};
inline int long_cmp(uint64_t hi, uint64_t lo, const LongThreshold &t)
{
    if (t.nbits == 0) return 0;
    if (t.nbits <= 64) {
        const uint64_t a = hi >> (64 - t.nbits);
        return a > t.ph ? 1 : (a < t.ph ? -1 : 0);
    }
    if (hi != t.ph) return hi > t.ph ? 1 : -1;
    const uint64_t b = lo >> (128 - t.nbits);
    return b > t.pl ? 1 : (b < t.pl ? -1 : 0);
}
// the list position of the k-th (from 1) member of the exact bin (hi, lo), LONG_NO_TIE when there are fewer
inline int32_t long_tie_position(const std::vector<LongKey> &c, uint64_t hi, uint64_t lo, int32_t k)
{
    int32_t seen = 0;
    for (size_t q = 0; q < c.size(); ++q)
        if (c[q].hi == hi && c[q].lo == lo && ++seen == k) return (int32_t)q;
    return LONG_NO_TIE;
}
inline LongThreshold long_threshold_model(const std::vector<LongKey> &c, int32_t top_n)
{
    LongThreshold t;
    t.k_rem = top_n, t.total = (int64_t)c.size();
    if (t.total <= top_n) { t.k_rem = (int32_t)t.total; return t; }
    for (int level = 0; level < LONG_SEL_LEVELS; ++level) {
        int64_t h[256] = {};
        for (const LongKey &k : c)
            if (long_cmp(k.hi, k.lo, t) == 0) ++h[level < 8 ? (k.hi >> (56 - 8 * level)) & 255u : (k.lo >> (56 - 8 * (level - 8))) & 255u];
        int64_t cum = 0;
        int sel = 0;
        for (int b = 255; b >= 0; --b) {
            if (cum + h[b] >= t.k_rem) { sel = b; break; }
            cum += h[b];
        }
        t.k_rem -= (int32_t)cum;
        if (level < 8) t.ph = (t.ph << 8) | (uint64_t)sel;
        else t.pl = (t.pl << 8) | (uint64_t)sel;
        t.nbits += 8;
        if (h[sel] <= LONG_SEL_CAP) break;
    }
    if (t.nbits == 128) t.q_tie = long_tie_position(c, t.ph, t.pl, t.k_rem);
    return t;
}

// The whole selection as the device runs it: threshold, collect (every key at or above it, the bin's members up to q_tie; the
// device appends in arrival order -- `arrival` != 0 shuffles the collected entries to stand for one), runs of LONG_RUN sorted,
// the planned merge passes between two buffers through long_pair_of / long_merge_range in steps of LONG_MERGE_ITEMS outputs,
// cut at top_n.  *collected_out: the entries collected (never more than long_capacity(top_n))
inline std::vector<LongKey> long_select_model(const std::vector<LongKey> &c, int32_t top_n, uint32_t arrival = 0, int64_t *collected_out = nullptr)
{
    const LongThreshold t = long_threshold_model(c, top_n);
    std::vector<LongKey> a;
    for (size_t q = 0; q < c.size(); ++q) {
        const int s = long_cmp(c[q].hi, c[q].lo, t);
        if (s > 0 || (s == 0 && (int64_t)q <= (int64_t)t.q_tie)) a.push_back(c[q]);
    }
    if (collected_out) *collected_out = (int64_t)a.size();
    uint64_t x = arrival;
    for (size_t i = a.size(); arrival != 0 && i > 1; --i) {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        std::swap(a[i - 1], a[(size_t)((x >> 33) % i)]);
    }
    const int64_t cnt = (int64_t)a.size();
    const auto first = [](const LongKey &p, const LongKey &q) { return long_key_lt(q, p); };
    for (int64_t r0 = 0; r0 < cnt; r0 += LONG_RUN) std::sort(a.begin() + r0, a.begin() + std::min(cnt, r0 + LONG_RUN), first);
    std::vector<LongKey> b(a.size());
    const int32_t passes = long_passes(long_capacity(top_n));
    for (int32_t p = 0; p < passes; ++p) {
        for (int64_t o = 0; o < cnt; o += LONG_MERGE_ITEMS) {
            const LongPair pr = long_pair_of(o, long_pass_width(p), cnt);
            const int64_t d = o - pr.base, left = pr.la + pr.lb - d;
            long_merge_range(a.data() + pr.base, pr.la, a.data() + pr.base + pr.la, pr.lb, d, left < LONG_MERGE_ITEMS ? left : LONG_MERGE_ITEMS,
                             b.data() + o);
        }
        a.swap(b);
    }
    if (cnt > top_n) a.resize((size_t)top_n);
    return a;
}

}  // namespace rwr
