// Host-side check of the group cap's plan (recommendersystems_amd/csrc/cap_plan.h), built against the header alone by
// tests/test_cap_plan.py: the order of the sort keys, the chunk and segment tables at the segment lengths that matter, the
// selection model against a brute-force sort for every m.  (The argument verdicts: tests/cpp/typed_call_check.cpp.)  Prints
// every failure and exits non-zero if there is one.
#include "cap_plan.h"

#include <algorithm>
#include <cstdio>
#include <map>
#include <random>
#include <string>
#include <tuple>
#include <vector>

using namespace rwr;

static int failures = 0;

static void fail(const std::string &what)
{
    if (++failures <= 40) std::printf("FAIL %s\n", what.c_str());
}

// ---- the key order ------------------------------------------------------------------------------------------------------------

static void check_keys()
{
    // labels first, rows inside a label; the largest label and row keep their bits
    const int32_t labels[] = {0, 1, 2, 255, 256, 65535, 1 << 20, 0x7FFFFFFF};
    const int32_t rows[] = {0, 1, 255, 256, 1 << 20, 0x7FFFFFFE};
    uint64_t prev = 0;
    bool first = true;
    for (int32_t lb : labels)
        for (int32_t r : rows) {
            const uint64_t k = cap_key(lb, r);
            if (cap_key_label(k) != lb || cap_key_row(k) != r) fail("key round trip " + std::to_string(lb) + "/" + std::to_string(r));
            if (!first && !(k > prev)) fail("key order at " + std::to_string(lb) + "/" + std::to_string(r));
            if (k >> cap_key_bits(lb) != 0 && cap_key_bits(lb) < 64) fail("key bits of label " + std::to_string(lb));
            prev = k, first = false;
        }
    if (cap_key_bits(0) != 33 || cap_key_bits(1) != 33 || cap_key_bits(2) != 34 || cap_key_bits(0x7FFFFFFF) != 63) fail("cap_key_bits");
    // the sorted keys of a list: groups contiguous, rows ascending inside, unlabelled rows left out
    std::mt19937 rng(5);
    for (int round = 0; round < 20; ++round) {
        const int32_t n = 1 + (int32_t)(rng() % 300);
        std::vector<int32_t> group_of((size_t)n), list;
        for (int32_t i = 0; i < n; ++i) {
            group_of[(size_t)i] = (int32_t)(rng() % 9) - 2;       // -2 .. 6
            if (rng() % 3) list.push_back(i);
        }
        const std::vector<uint64_t> keys = cap_sorted_keys(list.data(), (int32_t)list.size(), group_of.data());
        std::vector<std::pair<int32_t, int32_t>> want;
        for (int32_t r : list)
            if (group_of[(size_t)r] >= 0) want.push_back({group_of[(size_t)r], r});
        std::sort(want.begin(), want.end());
        if (keys.size() != want.size()) { fail("sorted keys: length"); continue; }
        for (size_t p = 0; p < keys.size(); ++p)
            if (cap_key_label(keys[p]) != want[p].first || cap_key_row(keys[p]) != want[p].second) { fail("sorted keys: entry"); break; }
        const std::vector<int32_t> start = cap_segment_starts(keys);
        if (start.back() != (int32_t)keys.size()) fail("segment starts: the end");
        for (size_t s = 0; s + 1 < start.size(); ++s) {
            if (start[s] >= start[s + 1]) fail("segment starts: empty segment");
            for (int32_t p = start[s]; p < start[s + 1]; ++p)
                if (cap_key_label(keys[(size_t)p]) != cap_key_label(keys[(size_t)start[s]])) fail("segment starts: two labels in one segment");
            if (s > 0 && cap_key_label(keys[(size_t)start[s]]) == cap_key_label(keys[(size_t)start[s] - 1])) fail("segment starts: a label split");
        }
    }
}

// ---- chunk and segment tables ---------------------------------------------------------------------------------------------------

static void check_tables(const std::string &name, const std::vector<int32_t> &lens, int32_t m, int32_t chunk)
{
    std::vector<int32_t> start(1, 0);
    for (int32_t len : lens)
        if (len > 0) start.push_back(start.back() + len);         // (a segment of length 0 does not exist in a sorted list)
    const int32_t nseg = (int32_t)start.size() - 1;
    const CapPlan pl = cap_plan(start.data(), nseg, m, chunk);
    // brute force: which positions are planned, and by which chunk
    const int32_t total = start.back();
    std::vector<int32_t> owner((size_t)total, -1);
    const size_t nchunks = pl.chunk_pos.size();
    if (pl.chunk_len.size() != nchunks || pl.chunk_seg.size() != nchunks) { fail(name + ": chunk table sizes"); return; }
    const size_t nplanned = pl.seg_pos.size();
    if (pl.seg_len.size() != nplanned || pl.seg_chunk0.size() != nplanned || pl.seg_nchunks.size() != nplanned) { fail(name + ": segment table sizes"); return; }
    for (size_t c = 0; c < nchunks; ++c) {
        if (pl.chunk_len[c] < 1 || pl.chunk_len[c] > chunk) { fail(name + ": chunk length"); return; }
        if (pl.chunk_seg[c] < 0 || (size_t)pl.chunk_seg[c] >= nplanned) { fail(name + ": chunk segment"); return; }
        for (int32_t p = pl.chunk_pos[c]; p < pl.chunk_pos[c] + pl.chunk_len[c]; ++p) {
            if (p < 0 || p >= total || owner[(size_t)p] != -1) { fail(name + ": chunks overlap or leave the list"); return; }
            owner[(size_t)p] = (int32_t)c;
        }
    }
    size_t planned = 0, singles = 0, multis = 0, msegs = 0;
    for (int32_t s = 0; s < nseg; ++s) {
        const int32_t len = start[(size_t)s + 1] - start[(size_t)s];
        const bool want = len > m;
        for (int32_t p = start[(size_t)s]; p < start[(size_t)s + 1]; ++p)
            if ((owner[(size_t)p] >= 0) != want) { fail(name + ": segment of length " + std::to_string(len) + " planned wrongly"); return; }
        if (!want) continue;
        if (planned >= nplanned) { fail(name + ": planned segments missing"); return; }
        const int32_t nc = (len + chunk - 1) / chunk;
        if (pl.seg_pos[planned] != start[(size_t)s] || pl.seg_len[planned] != len || pl.seg_nchunks[planned] != nc) { fail(name + ": segment entry"); return; }
        for (int32_t c = 0; c < nc; ++c) {
            const size_t id = (size_t)pl.seg_chunk0[planned] + (size_t)c;
            if (id >= nchunks || pl.chunk_seg[id] != (int32_t)planned || pl.chunk_pos[id] != start[(size_t)s] + c * chunk) { fail(name + ": a segment's chunks"); return; }
            if (c + 1 < nc && pl.chunk_len[id] != chunk) { fail(name + ": a short chunk inside a segment"); return; }
            if (nc == 1) {
                if (singles >= pl.single.size() || pl.single[singles++] != (int32_t)id) { fail(name + ": single list"); return; }
            } else {
                if (multis >= pl.multi.size() || pl.multi[multis] != (int32_t)id || pl.multi_mseg[multis] != (int32_t)msegs) { fail(name + ": multi list"); return; }
                ++multis;
            }
        }
        if (nc > 1) {
            if (msegs >= pl.mseg_first.size() || pl.mseg_first[msegs] != (int32_t)multis - nc || pl.mseg_count[msegs] != nc) { fail(name + ": multi segment entry"); return; }
            ++msegs;
        }
        ++planned;
    }
    if (planned != nplanned || singles != pl.single.size() || multis != pl.multi.size() || msegs != pl.mseg_first.size() ||
        pl.multi_mseg.size() != pl.multi.size() || pl.mseg_count.size() != pl.mseg_first.size())
        fail(name + ": surplus table entries");
}

static void check_all_tables()
{
    for (int32_t m = 1; m <= CAP_MAX; ++m)
        for (int32_t chunk : {CAP_CHUNK, 1, 3, 4, 64}) {
            const std::string tag = "m " + std::to_string(m) + " chunk " + std::to_string(chunk);
            const std::vector<int32_t> edge = {0, 1, m, m + 1, chunk - 1, chunk, chunk + 1, 3 * chunk + 1};
            for (int32_t len : edge) check_tables(tag + " one segment of " + std::to_string(len), {len}, m, chunk);
            check_tables(tag + " all edge lengths", edge, m, chunk);
            std::vector<int32_t> rev(edge.rbegin(), edge.rend());
            check_tables(tag + " all edge lengths reversed", rev, m, chunk);
            check_tables(tag + " no segment", {}, m, chunk);
            check_tables(tag + " every row its own label", std::vector<int32_t>(700, 1), m, chunk);
            check_tables(tag + " one label for everything", {2000}, m, chunk);
        }
    // all labels negative: no key, no segment, no chunk; the same through the key builder
    const std::vector<int32_t> rows = {0, 1, 2, 3, 4}, none(5, -1), one(5, 7), own = {4, 3, 2, 1, 0};
    if (!cap_sorted_keys(rows.data(), 5, none.data()).empty()) fail("all labels negative: keys");
    const std::vector<uint64_t> k1 = cap_sorted_keys(rows.data(), 5, one.data()), k2 = cap_sorted_keys(rows.data(), 5, own.data());
    const std::vector<int32_t> s1 = cap_segment_starts(k1), s2 = cap_segment_starts(k2), s0 = cap_segment_starts({});
    if (s0.size() != 1 || s0[0] != 0) fail("no keys: segment starts");
    if (s1.size() != 2 || s1[0] != 0 || s1[1] != 5) fail("one label: segment starts");
    if (s2.size() != 6) fail("every row its own label: segment starts");
    const CapPlan p1 = cap_plan(s1.data(), 1, 2, CAP_CHUNK), p2 = cap_plan(s2.data(), 5, 1, CAP_CHUNK), p0 = cap_plan(s0.data(), 0, 1, CAP_CHUNK);
    if (p1.single.size() != 1 || p1.chunk_len[0] != 5 || !p1.multi.empty()) fail("one label: plan");
    if (!p2.chunk_pos.empty() || !p0.chunk_pos.empty()) fail("segments that can lose nobody are planned");
}

// ---- the selection model ----------------------------------------------------------------------------------------------------------

static void check_selection()
{
    std::mt19937 rng(17);
    for (int round = 0; round < 400; ++round) {
        const int32_t n = 1 + (int32_t)(rng() % 90);
        const int kind = round % 4;                               // 0: random scores, 1: all zero, 2: few distinct scores, 3: equal (score, id) pairs
        std::vector<double> col((size_t)n);
        std::vector<int64_t> id((size_t)n);
        for (int32_t i = 0; i < n; ++i) {
            col[(size_t)i] = kind == 1 ? 0.0 : kind == 0 ? (double)(rng() % 1000) / 7.0 : (double)(rng() % 3);
            if (rng() % 5 == 0) col[(size_t)i] = -1.0;            // excluded
            if (kind == 1 && rng() % 7 == 0) col[(size_t)i] = -0.0;
            id[(size_t)i] = kind == 3 ? (int64_t)(rng() % 4) - 2 : (int64_t)(rng() % 100000) - 50000;
        }
        // a run of the sorted keys: a subset of the rows, ascending
        std::vector<uint64_t> keys;
        for (int32_t i = 0; i < n; ++i)
            if (rng() % 4) keys.push_back(cap_key(3, i));
        const int32_t len = (int32_t)keys.size();
        // brute force: the live cells sorted by (score desc, id desc, row asc)
        std::vector<std::tuple<double, int64_t, int32_t>> live;
        for (uint64_t k : keys) {
            const int32_t r = cap_key_row(k);
            if (col[(size_t)r] >= 0.0) live.push_back({col[(size_t)r] + 0.0, id[(size_t)r], r});
        }
        std::sort(live.begin(), live.end(), [](const auto &a, const auto &b) {
            if (std::get<0>(a) != std::get<0>(b)) return std::get<0>(a) > std::get<0>(b);
            if (std::get<1>(a) != std::get<1>(b)) return std::get<1>(a) > std::get<1>(b);
            return std::get<2>(a) < std::get<2>(b);
        });
        for (int32_t m = 1; m <= CAP_MAX; ++m)
            for (int32_t chunk : {CAP_CHUNK, 1, 5}) {
                const CapKey thr = cap_threshold(col.data(), 1, id.data(), keys.data(), 0, len, m, chunk);
                const std::string tag = "selection round " + std::to_string(round) + " m " + std::to_string(m) + " chunk " + std::to_string(chunk);
                if ((int32_t)live.size() < m) {
                    if (thr.hi != 0 || thr.lo != 0 || thr.rw != 0) fail(tag + ": fewer than m live cells must give the bottom key");
                } else {
                    const auto &w = live[(size_t)m - 1];
                    const CapKey want = cap_rank_key(std::get<0>(w), std::get<1>(w), std::get<2>(w));
                    if (thr.hi != want.hi || thr.lo != want.lo || thr.rw != want.rw) fail(tag + ": the m-th best key");
                }
                // kept = not worse than the threshold: exactly the first min(m, live) of the brute-force order
                for (size_t at = 0; at < live.size(); ++at) {
                    const CapKey k = cap_rank_key(std::get<0>(live[at]), std::get<1>(live[at]), std::get<2>(live[at]));
                    if (cap_better(thr, k) != (at >= (size_t)m)) { fail(tag + ": kept set"); break; }
                }
            }
    }
    // the order of the keys themselves
    const CapKey a = cap_rank_key(1.0, 5, 9), b = cap_rank_key(1.0, 5, 8), c = cap_rank_key(1.0, 6, 9), d = cap_rank_key(2.0, -7, 9);
    if (!cap_better(b, a) || !cap_better(c, b) || !cap_better(d, c) || cap_better(a, a)) fail("rank key order");
    if (cap_rank_key(-0.0, 1, 1).hi != cap_rank_key(0.0, 1, 1).hi) fail("-0.0 and +0.0 are one score");
    const CapKey top{~0ull, ~0ull, ~0u}, bottom{0, 0, 0}, lo = cap_rank_key(0.0, INT64_MIN, 0x7FFFFFFF), hi = cap_rank_key(1e308, INT64_MAX, 0);
    if (!cap_better(top, hi) || !cap_better(lo, bottom) || !cap_is_top(top) || cap_is_top(hi)) fail("sentinels");
}

int main()
{
    check_keys();
    check_all_tables();
    check_selection();
    std::printf("%d failures\n", failures);
    return failures != 0;
}
