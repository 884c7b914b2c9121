// Host-side check of the evaluation plan (recommendersystems_amd/csrc/eval_plan.h), built against the header alone by
// tests/test_eval_plan.py: the laid-out test sets of hand-made and random cases against a direct restatement (std::set per
// slot), the slot and tile-group offsets, the buffer sizes, the layout of a tile group's hit lists and counters from its hit
// counts, then every validation verdict with the set it reports.  Prints every failure and exits non-zero if there is one.
#include "eval_plan.h"

#include <cstdio>
#include <random>
#include <set>
#include <string>
#include <vector>

using namespace rwr;

static int failures = 0;

static void fail(const std::string &what)
{
    if (++failures <= 40) std::printf("FAIL %s\n", what.c_str());
}

using Sets = std::vector<std::vector<int64_t>>;

static void flatten(const Sets &sets, std::vector<int64_t> &ptr, std::vector<int64_t> &ids)
{
    ptr.assign(1, 0);
    ids.clear();
    for (const auto &s : sets) {
        ids.insert(ids.end(), s.begin(), s.end());
        ptr.push_back((int64_t)ids.size());
    }
}

// K = sets.size() vectors dealt to ntiles tiles of G slots as the driver deals them (vector k in slot
// (k % ntiles) * G + k / ntiles, the rest padding), TG tiles per tile group.  Returns the number of ids laid out.
static size_t check_case(const std::string &name, const Sets &sets, int G, int TG)
{
    const int32_t K = (int32_t)sets.size();
    const size_t ntiles = ((size_t)K + G - 1) / G, nslots = ntiles * G, per_group = (size_t)TG * G;
    std::vector<int32_t> slot_k(nslots, -1);
    for (int32_t k = 0; k < K; ++k) slot_k[(size_t)(k % ntiles) * G + (size_t)(k / ntiles)] = k;
    std::vector<int64_t> ptr, ids;
    flatten(sets, ptr, ids);
    int64_t hits = 0;
    double sum = 0;
    const EvalPlan p = eval_plan(nslots, slot_k.data(), per_group, K, ptr.data(), ids.empty() ? nullptr : ids.data(), &hits, &sum);
    if (p.check.verdict != EVAL_OK) { fail(name + ": verdict " + std::to_string((int)p.check.verdict)); return 0; }
    const size_t ngroups = per_group ? (nslots + per_group - 1) / per_group : 0;
    if (p.slot_off.size() != nslots + 1 || p.slot_off[0] != 0 || p.slot_off[nslots] != (int64_t)p.ids.size()) {
        fail(name + ": slot offsets");
        return 0;
    }
    if (p.group_off.size() != ngroups + 1 || p.group_off[0] != 0 || p.group_off[ngroups] != (int64_t)p.ids.size()) {
        fail(name + ": group offsets");
        return 0;
    }
    if (p.n_ids != p.ids.size() || p.n_off != nslots + 1 || p.n_out != (size_t)K || p.n_group_slots != std::min(per_group, nslots))
        fail(name + ": buffer sizes");
    for (size_t slot = 0; slot < nslots; ++slot) {
        const int64_t a = p.slot_off[slot], b = p.slot_off[slot + 1];
        if (a > b) { fail(name + ": slot offsets decrease"); return p.ids.size(); }
        // the direct restatement: HashSet<long> of the slot's vector, ascending
        std::set<int64_t> want;
        if (slot_k[slot] >= 0) want.insert(sets[(size_t)slot_k[slot]].begin(), sets[(size_t)slot_k[slot]].end());
        const std::vector<int64_t> got(p.ids.begin() + a, p.ids.begin() + b);
        if (got != std::vector<int64_t>(want.begin(), want.end()))
            fail(name + ": slot " + std::to_string(slot) + " does not hold its set sorted and without duplicates");
    }
    for (size_t gi = 0; gi < ngroups; ++gi)
        if (p.group_off[gi] != p.slot_off[gi * per_group]) fail(name + ": group " + std::to_string(gi) + " does not start at its first slot");
    return p.ids.size();
}

// hit counts of one tile group against a direct restatement of the layout
static void check_layout(const std::string &name, const std::vector<int32_t> &cnt, int G, size_t lds_bytes)
{
    const size_t S = cnt.size();
    const EvalGroupLayout L = eval_group_layout(cnt.data(), S, G, lds_bytes);
    if (L.bad) { fail(name + ": bad"); return; }
    if (L.hit_off.size() != S + 1 || L.hit_off[0] != 0) { fail(name + ": hit offsets"); return; }
    int64_t tot = 0, longest = 0;
    std::vector<int32_t> longs;
    for (size_t s = 0; s < S; ++s) {
        if (L.hit_off[s] != tot) fail(name + ": hit offset of slot " + std::to_string(s));
        // the slot's counters [hit_off + slot, hit_off + slot + cnt + 1) do not overlap the next slot's
        if (s + 1 < S && L.hit_off[s] + (int64_t)s + cnt[s] + 1 != L.hit_off[s + 1] + (int64_t)s + 1) fail(name + ": counters overlap");
        tot += cnt[s];
        if (cnt[s] > EVAL_SORT_SLOTS) { longs.push_back((int32_t)s); longest = std::max<int64_t>(longest, cnt[s]); }
    }
    if (L.hit_off[S] != tot || L.n_hits != tot || L.n_counters != tot + (int64_t)S) fail(name + ": totals");
    if (L.long_slots != longs || L.max_long != longest) fail(name + ": long slots");
    const size_t tiles = (S + (size_t)G - 1) / (size_t)G;
    if (L.tile_lds.size() != tiles) { fail(name + ": tiles"); return; }
    for (size_t t = 0; t < tiles; ++t) {
        uint64_t h = 0, slots = 0;
        for (size_t s = t * G; s < std::min(S, (t + 1) * G); ++s) { h += (uint64_t)cnt[s]; ++slots; }
        const bool fits = h * 16 + (h + slots) * 4 <= lds_bytes;
        if ((L.tile_lds[t] != 0) != fits) fail(name + ": LDS verdict of tile " + std::to_string(t));
    }
}

static void check_verdict(const std::string &name, int32_t K, const int64_t *ptr, const int64_t *ids, const void *hits, const void *sum,
                          EvalVerdict v, int32_t bad_k)
{
    const EvalCheck c = eval_check(K, ptr, ids, hits, sum);
    if (c.verdict != v || (bad_k >= 0 && c.bad_k != bad_k))
        fail(name + ": verdict " + std::to_string((int)c.verdict) + " at set " + std::to_string(c.bad_k));
    // the plan carries the same verdict and plans nothing
    std::vector<int32_t> slot_k((size_t)(K > 0 ? K : 0));
    for (int32_t k = 0; k < K; ++k) slot_k[(size_t)k] = k;
    const EvalPlan p = eval_plan(slot_k.size(), slot_k.data(), 1, K, ptr, ids, hits, sum);
    if (p.check.verdict != v || (v != EVAL_OK && !p.ids.empty())) fail(name + ": the plan's verdict");
    if (p.slot_off.size() != slot_k.size() + 1) fail(name + ": the plan's offsets");
}

int main()
{
    // empty sets, duplicates, ids no node would carry (negative, huge), one set
    if (check_case("empty", {{}}, 1, 1) != 0) fail("empty: ids laid out");
    if (check_case("only empty", {{}, {}, {}}, 2, 1) != 0) fail("only empty sets");
    if (check_case("duplicates", {{5, 5, 5, 2, 5, 2}}, 1, 1) != 2) fail("duplicates: not two ids");
    if (check_case("extremes", {{INT64_MAX, INT64_MIN, 0, -1, INT64_MAX}}, 4, 1) != 4) fail("extremes");
    if (check_case("empty between", {{3, 1}, {}, {1, 3, 1}}, 4, 1) != 4) fail("empty between");
    // the same sets on either side of a tile-group boundary, every group starting at its own first slot
    check_case("two groups", {{3, 1}, {3, 1}, {9}, {1, 3, 3}}, 2, 1);
    check_case("two groups of two tiles", {{3}, {6, 3}, {2}, {3, 3}, {4}, {6}, {}, {0}, {8, 8}}, 2, 2);
    // padding slots at every tile width: 5 vectors in tiles of G (G = 64: 59 padding slots), one tile group or several
    const Sets five = {{1, 2}, {3}, {}, {8, 4, 6, 4}, {5, 0, 1}};
    for (int G = 1; G <= 64; G *= 2)
        for (int TG : {1, 2, 8})
            if (check_case("padding G=" + std::to_string(G) + " TG=" + std::to_string(TG), five, G, TG) != 9) fail("padding: ids");

    std::mt19937_64 rng(11);
    for (int it = 0; it < 400; ++it) {
        const int K = (int)(rng() % 12);
        Sets sets((size_t)K);
        for (auto &s : sets) {
            const int len = (int)(rng() % 9);
            for (int j = 0; j < len; ++j) s.push_back((int64_t)(rng() % 12) - 3);
        }
        const int G = 1 << (rng() % 7), TG = 1 + (int)(rng() % 3);
        check_case("random " + std::to_string(it), sets, G, TG);
    }

    // a tile group's layout: no hits, lists at the one-workgroup sort's limit and one past it, tiles at the LDS budget's edge
    check_layout("no hits", {0, 0, 0, 0}, 2, EVAL_LDS_BYTES);
    check_layout("sort limit", {EVAL_SORT_SLOTS, EVAL_SORT_SLOTS + 1, 0, 7}, 1, EVAL_LDS_BYTES);
    check_layout("lds edge", {3, 0, 2, 2}, 2, 3 * 16 + 5 * 4);          // tile 0 fits exactly, tile 1 (4 hits) does not
    check_layout("lds edge - 1", {3, 0, 1, 1}, 2, 3 * 16 + 5 * 4 - 1);
    {
        const EvalGroupLayout L = eval_group_layout(std::vector<int32_t>{3, 0, 2, 2}.data(), 4, 2, 3 * 16 + 5 * 4);
        if (L.tile_lds.size() != 2 || !L.tile_lds[0] || L.tile_lds[1]) fail("lds edge: verdicts");
        const EvalGroupLayout B = eval_group_layout(std::vector<int32_t>{3, -1}.data(), 2, 2);
        if (!B.bad) fail("negative count not refused");
    }
    for (int it = 0; it < 300; ++it) {
        const int G = 1 << (rng() % 7), tiles = 1 + (int)(rng() % 3);
        std::vector<int32_t> cnt((size_t)G * tiles);
        for (auto &c : cnt) {
            const int k = (int)(rng() % 10);
            c = k == 0 ? EVAL_SORT_SLOTS : k == 1 ? EVAL_SORT_SLOTS + 1 + (int32_t)(rng() % 100) : k < 5 ? 0 : (int32_t)(rng() % 200);
        }
        check_layout("random layout " + std::to_string(it), cnt, G, (size_t)(rng() % (128 * 1024)));
    }

    // every validation verdict, the first offender reported, in the order of the checks
    {
        int64_t hits = 0;
        double sum = 0;
        const int64_t ids[4] = {7, 7, -2, 9};
        const int64_t ok[4] = {0, 2, 2, 4}, ptr0[4] = {1, 2, 2, 4}, dec[4] = {0, 2, 1, 4}, dec_end[4] = {0, 2, 2, 1};
        const int64_t zero[4] = {0, 0, 0, 0};
        check_verdict("ok", 3, ok, ids, &hits, &sum, EVAL_OK, -1);
        check_verdict("K = 0", 0, nullptr, nullptr, nullptr, nullptr, EVAL_OK, -1);
        check_verdict("NULL ptr", 3, nullptr, ids, &hits, &sum, EVAL_NULL_PTR, -1);
        check_verdict("NULL n_hits", 3, ok, ids, nullptr, &sum, EVAL_NULL_OUT, -1);
        check_verdict("NULL sum_precision", 3, ok, ids, &hits, nullptr, EVAL_NULL_OUT, -1);
        check_verdict("ptr[0]", 3, ptr0, ids, &hits, &sum, EVAL_BAD_PTR0, -1);
        check_verdict("decrease", 3, dec, ids, &hits, &sum, EVAL_PTR_DECREASES, 1);
        check_verdict("decrease at the end", 3, dec_end, ids, &hits, &sum, EVAL_PTR_DECREASES, 2);
        check_verdict("NULL ids", 3, ok, nullptr, &hits, &sum, EVAL_NULL_IDS, -1);
        check_verdict("NULL ids, empty sets", 3, zero, nullptr, &hits, &sum, EVAL_OK, -1);
        // (the ids of a set that is too large are never read: the verdict comes from the pointer array)
        const int64_t big[4] = {0, 1, 1 + EVAL_SET_MAX, 2 + EVAL_SET_MAX}, huge[4] = {0, 1, 2 + EVAL_SET_MAX, 3 + EVAL_SET_MAX};
        check_verdict("set too large", 3, huge, ids, &hits, &sum, EVAL_SET_TOO_LARGE, 1);
        const EvalCheck at_max = eval_check(3, big, ids, &hits, &sum);
        if (at_max.verdict != EVAL_OK) fail("a set of exactly INT32_MAX ids is legal");
        // the pointers' presence is reported before the pointer array, that before the id array, that before a set's size
        check_verdict("order: outputs before ptr[0]", 3, ptr0, nullptr, nullptr, &sum, EVAL_NULL_OUT, -1);
        check_verdict("order: decrease before NULL ids", 3, dec, nullptr, &hits, &sum, EVAL_PTR_DECREASES, 1);
        check_verdict("order: NULL ids before size", 3, huge, nullptr, &hits, &sum, EVAL_NULL_IDS, -1);
    }
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
