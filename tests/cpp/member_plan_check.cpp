// Host-side check of the typed ends' plan (recommendersystems_amd/csrc/member_plan.h), built against the headers alone by
// tests/test_member_plan.py: the (slot, member) pairs of hand-made and random cases against a direct walk over the sets (how
// often each row of each slot is named), the pairs' order and group offsets, then the argument verdicts that
// rwr_recommend_typed_eval_batch and rwr_recommend_restart_typed_batch add, against a plain restatement of their header
// comments, first finding first.  Prints every failure and exits non-zero if there is one.
#include "member_plan.h"

#include <algorithm>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

using namespace rwr;

static int failures = 0;

static void fail(const std::string &what)
{
    if (++failures <= 40) std::printf("FAIL %s\n", what.c_str());
}

using Sets = std::vector<std::vector<int32_t>>;

static void flatten(const Sets &sets, std::vector<int64_t> &ptr, std::vector<int32_t> &idx)
{
    ptr.assign(1, 0);
    idx.clear();
    for (const auto &s : sets) {
        idx.insert(idx.end(), s.begin(), s.end());
        ptr.push_back((int64_t)idx.size());
    }
}

// K = sets.size() vectors over n nodes; slot_k: the slot assignment (-1 = padding), per_group slots per tile group.
// Returns the number of pairs.
static size_t check_slots(const std::string &name, int32_t n, const Sets &sets, const std::vector<int32_t> &slot_k, size_t per_group)
{
    const int32_t K = (int32_t)sets.size();
    const size_t nslots = slot_k.size();
    std::vector<int64_t> ptr;
    std::vector<int32_t> idx;
    flatten(sets, ptr, idx);
    const MemberPlan p = member_plan(n, nslots, slot_k.data(), per_group, K, ptr.data(), idx.empty() ? nullptr : idx.data());
    if (p.check.verdict != EXCLUDE_OK) { fail(name + ": verdict " + std::to_string((int)p.check.verdict)); return 0; }
    const size_t P = p.pair_slot.size(), ngroups = (nslots + per_group - 1) / per_group;
    if (p.pair_row.size() != P) { fail(name + ": table lengths"); return 0; }
    if (p.group_off.size() != ngroups + 1 || p.group_off[0] != 0 || p.group_off[ngroups] != (int64_t)P) {
        fail(name + ": group offsets");
        return 0;
    }
    // the direct walk: want[slot][row] = how often the slot's set names that row; the sets in slot order give the expected
    // sequence of rows as well
    std::vector<std::vector<int32_t>> want(nslots, std::vector<int32_t>((size_t)n, 0)), got(nslots, std::vector<int32_t>((size_t)n, 0));
    std::vector<int32_t> want_rows;
    size_t want_pairs = 0;
    for (size_t slot = 0; slot < nslots; ++slot)
        if (slot_k[slot] >= 0 && slot_k[slot] < K)
            for (int32_t i : sets[(size_t)slot_k[slot]]) {
                ++want[slot][(size_t)i];
                want_rows.push_back(i);
                ++want_pairs;
            }
    if (P != want_pairs) fail(name + ": " + std::to_string(P) + " pairs, " + std::to_string(want_pairs) + " expected");
    if (p.pair_row != want_rows) fail(name + ": rows not in slot order, set order");
    for (size_t gi = 0; gi < ngroups; ++gi) {
        if (p.group_off[gi] > p.group_off[gi + 1]) { fail(name + ": group offsets decrease"); return P; }
        const size_t in_group = std::min(per_group, nslots - gi * per_group);
        for (int64_t j = p.group_off[gi]; j < p.group_off[gi + 1]; ++j) {
            const int32_t ls = p.pair_slot[(size_t)j], row = p.pair_row[(size_t)j];
            if (ls < 0 || (size_t)ls >= in_group) { fail(name + ": slot outside its group"); return P; }
            if (j > p.group_off[gi] && ls < p.pair_slot[(size_t)j - 1]) fail(name + ": pairs not ordered by slot");
            if (row < 0 || row >= n) { fail(name + ": row outside [0, n)"); return P; }
            const size_t slot = gi * per_group + (size_t)ls;
            if (slot_k[slot] < 0) fail(name + ": pair of a padding slot");
            ++got[slot][(size_t)row];
        }
    }
    for (size_t slot = 0; slot < nslots; ++slot)
        if (got[slot] != want[slot]) { fail(name + ": slot " + std::to_string(slot) + " does not name its set's members"); break; }
    return P;
}

// the driver's dealing: vector k in slot (k % ntiles) * G + k / ntiles, the rest padding, TG tiles per tile group
static size_t check_case(const std::string &name, int32_t n, const Sets &sets, int G, int TG)
{
    const int32_t K = (int32_t)sets.size();
    const size_t ntiles = ((size_t)K + G - 1) / G, nslots = ntiles * G;
    std::vector<int32_t> slot_k(nslots, -1);
    for (int32_t k = 0; k < K; ++k) slot_k[(size_t)(k % ntiles) * G + (size_t)(k / ntiles)] = k;
    return check_slots(name, n, sets, slot_k, (size_t)TG * G);
}

// ---- the verdicts, restated ------------------------------------------------------------------------------------------------

struct EvalArgs {
    bool have_graph;
    int32_t n, K;
    const int32_t *seeds;
    int32_t cand_type;
    uint32_t mask;
    const int64_t *test_ptr, *test_ids;
    const void *n_hits, *sum_precision;
};

// rwr.h, rwr_recommend_typed_eval_batch: NULL g first, K == 0 a no-op, then K, the seeds' presence, cand_type, the mask, every
// seed; then test_ptr, the result arrays, test_ptr[0], the first decrease, test_ids, the first set that is too large
static void check_eval_verdict(const std::string &name, const EvalArgs &a)
{
    TypedVerdict tv = TYPED_OK;
    int32_t bad_k = -1, bad_seed = 0;
    if (!a.have_graph) tv = TYPED_NULL_GRAPH;
    else if (a.K < 0) tv = TYPED_NEGATIVE_K;
    else if (a.K == 0) tv = TYPED_NOOP;
    else if (!a.seeds) tv = TYPED_NULL_ARG;
    else if (a.cand_type < 0 || a.cand_type > 255) tv = TYPED_BAD_CAND_TYPE;
    else if (a.mask & ~0xFFu) tv = TYPED_BAD_MASK;
    else
        for (int32_t k = 0; k < a.K; ++k)
            if (a.seeds[k] < 0 || a.seeds[k] >= a.n) { tv = TYPED_SEED_RANGE, bad_k = k, bad_seed = a.seeds[k]; break; }
    EvalVerdict ev = EVAL_OK;
    int32_t ev_k = -1;
    if (tv == TYPED_OK) {
        if (!a.test_ptr) ev = EVAL_NULL_PTR;
        else if (!a.n_hits || !a.sum_precision) ev = EVAL_NULL_OUT;
        else if (a.test_ptr[0] != 0) ev = EVAL_BAD_PTR0;
        else {
            for (int32_t k = 0; k < a.K && ev == EVAL_OK; ++k)
                if (a.test_ptr[k + 1] < a.test_ptr[k]) ev = EVAL_PTR_DECREASES, ev_k = k;
            if (ev == EVAL_OK && a.test_ptr[a.K] > 0 && !a.test_ids) ev = EVAL_NULL_IDS;
            for (int32_t k = 0; k < a.K && ev == EVAL_OK; ++k)
                if (a.test_ptr[k + 1] - a.test_ptr[k] > 0x7FFFFFFFll) ev = EVAL_SET_TOO_LARGE, ev_k = k;
        }
    }
    const TypedEvalCheck c = typed_eval_check(a.have_graph, a.n, a.seeds, a.K, a.cand_type, a.mask, a.test_ptr, a.test_ids,
                                              a.n_hits, a.sum_precision);
    if (c.typed.verdict != tv || (tv == TYPED_SEED_RANGE && (c.typed.bad_k != bad_k || c.typed.bad_seed != bad_seed)))
        fail(name + ": typed verdict " + std::to_string((int)c.typed.verdict) + ", expected " + std::to_string((int)tv));
    if (c.eval.verdict != ev || (ev_k >= 0 && c.eval.bad_k != ev_k))
        fail(name + ": eval verdict " + std::to_string((int)c.eval.verdict) + ", expected " + std::to_string((int)ev));
    if (c.typed.verdict == TYPED_BAD_TOP_N || c.typed.verdict == TYPED_TOP_N_LIMIT) fail(name + ": a top_n verdict");
}

// rwr.h, rwr_recommend_restart_typed_batch: top_n < 1, cand_type, the mask, then the limit
static void check_restart_verdict(int32_t top_n, int32_t top_n_max, int32_t cand_type, uint32_t mask)
{
    TypedVerdict want = TYPED_OK;
    if (top_n < 1) want = TYPED_BAD_TOP_N;
    else if (cand_type < 0 || cand_type > 255) want = TYPED_BAD_CAND_TYPE;
    else if (mask & ~0xFFu) want = TYPED_BAD_MASK;
    else if (top_n > top_n_max) want = TYPED_TOP_N_LIMIT;
    const TypedVerdict got = restart_typed_check(top_n, top_n_max, cand_type, mask);
    if (got != want)
        fail("restart verdict top_n " + std::to_string(top_n) + " cand " + std::to_string(cand_type) + " mask " + std::to_string(mask) +
             ": " + std::to_string((int)got) + ", expected " + std::to_string((int)want));
}

int main()
{
    // one member, a member twice, an empty set, only empty sets
    if (check_case("one", 9, {{3}}, 1, 1) != 1) fail("one: not one pair");
    if (check_case("twice", 9, {{3, 4, 3}, {1}}, 2, 1) != 4) fail("twice: a member listed twice gives its pair twice");
    if (check_case("empty set", 9, {{}, {4}, {}}, 4, 1) != 1) fail("empty set");
    if (check_case("only empty", 9, {{}, {}}, 2, 1) != 0) fail("only empty sets");
    if (check_case("no vector", 9, {}, 4, 2) != 0) fail("no vector");
    // padding slots: 5 vectors in tiles of 4 (3 padding slots), in tiles of 64 (59), one tile group or one per tile
    const Sets five = {{1, 2}, {3}, {}, {8, 4, 6}, {5, 0, 1}};
    for (int G : {1, 2, 4, 64})
        for (int TG : {1, 2, 8}) check_case("padding G=" + std::to_string(G) + " TG=" + std::to_string(TG), 9, five, G, TG);
    // the same members on either side of a group boundary, every group's pairs counted from the group's own first slot
    check_case("two groups", 9, {{3, 1}, {3, 1}, {3}, {1, 3}}, 2, 1);
    check_case("two groups of two tiles", 9, {{3}, {6, 3}, {2}, {3, 3}, {4}, {6}, {1}, {0}, {8}}, 2, 2);
    // the vector-by-vector fallback's assignment: slot k = vector k, every slot its own group
    {
        std::vector<int32_t> slot_k = {0, 1, 2, 3, 4};
        if (check_slots("one slot per group", 9, five, slot_k, 1) != 9) fail("one slot per group: not nine pairs");
    }

    std::mt19937_64 rng(11);
    for (int it = 0; it < 400; ++it) {
        const int32_t n = 1 + (int32_t)(rng() % 12);
        const int K = (int)(rng() % 11);
        Sets sets((size_t)K);
        for (auto &s : sets) {
            const int len = (int)(rng() % 6);
            for (int j = 0; j < len; ++j) s.push_back((int32_t)(rng() % (uint64_t)n));
        }
        const int G = 1 << (rng() % 4), TG = 1 + (int)(rng() % 3);
        check_case("random " + std::to_string(it), n, sets, G, TG);
        // ... and a random assignment: the vectors shuffled over the slots of extra padding, a last group that is not full
        const size_t nslots = (size_t)K + (size_t)(rng() % 7);
        if (nslots == 0) continue;
        std::vector<int32_t> slot_k(nslots, -1);
        for (int k = 0; k < K; ++k) slot_k[(size_t)k] = k;
        std::shuffle(slot_k.begin(), slot_k.end(), rng);
        check_slots("shuffled " + std::to_string(it), n, sets, slot_k, 1 + (size_t)(rng() % 5));
    }

    // bad sets plan nothing and carry exclude_check's verdict
    {
        const int32_t idx[4] = {0, 3, 4, 1}, slot_k[3] = {0, 1, 2};
        const int64_t ok[4] = {0, 2, 2, 4}, dec[4] = {0, 2, 1, 4};
        const MemberPlan a = member_plan(4, 3, slot_k, 2, 3, ok, idx);
        if (a.check.verdict != EXCLUDE_BAD_INDEX || a.check.bad_k != 2 || a.check.bad_index != 4 || !a.pair_slot.empty() ||
            !a.pair_row.empty() || a.group_off != std::vector<int64_t>(3, 0))
            fail("index n: not refused whole");
        const MemberPlan b = member_plan(5, 3, slot_k, 2, 3, dec, idx);
        if (b.check.verdict != EXCLUDE_PTR_DECREASES || !b.pair_slot.empty()) fail("decrease: not refused whole");
        const MemberPlan c = member_plan(5, 3, slot_k, 2, 3, ok, nullptr);
        if (c.check.verdict != EXCLUDE_NULL_IDX || !c.pair_slot.empty()) fail("NULL idx: not refused whole");
    }

    // the verdicts of the evaluating typed entry: every finding alone, then random combinations (the first one wins)
    {
        const int32_t seeds[3] = {0, 4, 2}, bad_seeds[3] = {0, 5, -1};
        const int64_t ok[4] = {0, 2, 2, 4}, ptr0[4] = {1, 2, 2, 4}, dec[4] = {0, 2, 1, 4}, big[4] = {0, 2, 0x80000002ll, 0x80000003ll};
        const int64_t ids[4] = {7, 7, 9, -1}, zero[4] = {0, 0, 0, 0};
        int64_t h[3];
        double sp[3];
        const EvalArgs good{true, 5, 3, seeds, 1, 0x0cu, ok, ids, h, sp};
        check_eval_verdict("good", good);
        EvalArgs a = good;
        a.have_graph = false; check_eval_verdict("NULL graph", a); a = good;
        a.K = -1; check_eval_verdict("negative K", a); a = good;
        a.K = 0; check_eval_verdict("K = 0", a);
        a.seeds = nullptr, a.test_ptr = nullptr, a.n_hits = nullptr; check_eval_verdict("K = 0 with nothing", a); a = good;
        a.seeds = nullptr; check_eval_verdict("NULL seeds", a); a = good;
        a.cand_type = 256; check_eval_verdict("cand_type 256", a); a.cand_type = -1; check_eval_verdict("cand_type -1", a); a = good;
        a.cand_type = 255, a.mask = 0xffu; check_eval_verdict("the widest legal type and mask", a); a = good;
        a.mask = 0x100u; check_eval_verdict("mask bit 8", a); a = good;
        a.seeds = bad_seeds; check_eval_verdict("seed range", a); a = good;
        a.test_ptr = nullptr; check_eval_verdict("NULL test_ptr", a); a = good;
        a.n_hits = nullptr; check_eval_verdict("NULL n_hits", a); a = good;
        a.sum_precision = nullptr; check_eval_verdict("NULL sum_precision", a); a = good;
        a.test_ptr = ptr0; check_eval_verdict("test_ptr[0]", a); a = good;
        a.test_ptr = dec; check_eval_verdict("decrease", a); a = good;
        a.test_ids = nullptr; check_eval_verdict("NULL test_ids", a);
        a.test_ptr = zero; check_eval_verdict("NULL test_ids, empty sets", a); a = good;
        a.test_ptr = big; check_eval_verdict("set too large", a); a = good;
        // the typed arguments come before the test sets
        a.seeds = bad_seeds, a.test_ptr = nullptr; check_eval_verdict("seed range before NULL test_ptr", a); a = good;
        a.mask = 0x100u, a.n_hits = nullptr; check_eval_verdict("mask before NULL n_hits", a); a = good;
        const int64_t *ptrs[5] = {ok, ptr0, dec, big, nullptr};
        for (int it = 0; it < 4000; ++it) {
            EvalArgs r = good;
            r.have_graph = rng() % 8 != 0;
            r.K = (int32_t)(rng() % 5) - 1;
            r.seeds = rng() % 6 == 0 ? nullptr : (rng() % 3 == 0 ? bad_seeds : seeds);
            r.cand_type = (int32_t)(rng() % 260) - 2;
            r.mask = rng() % 3 == 0 ? (uint32_t)(rng() % 0x400u) : 0x0cu;
            r.test_ptr = ptrs[rng() % 5];
            r.test_ids = rng() % 4 == 0 ? nullptr : ids;
            r.n_hits = rng() % 6 == 0 ? nullptr : h;
            r.sum_precision = rng() % 6 == 0 ? nullptr : sp;
            check_eval_verdict("random verdict " + std::to_string(it), r);
        }
    }
    // ... and of the typed restart entry
    for (int32_t top_n : {-1, 0, 1, 10, 1024, 1025, 0x7FFFFFFF})
        for (int32_t cand : {-1, 0, 1, 255, 256})
            for (uint32_t mask : {0u, 0x0cu, 0xffu, 0x100u, 0x80000000u}) check_restart_verdict(top_n, 1024, cand, mask);

    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
