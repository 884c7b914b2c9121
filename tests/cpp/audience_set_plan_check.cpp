// CPU check of recommendersystems_amd/csrc/audience_set_plan.h against brute-force loops: the ladder's order with the status
// and message of every refusal, the merge of repeated members, the (slot, row, weight) pairs across a tile-group boundary and
// the exclusion tables of sets.  Built against the header alone.  Without arguments it runs the checks and prints
// "<k> failures"; "messages" prints one line "<verdict> <status> <text>" per refusal of a fixed faulty call, which
// tests/test_audience_set_abi.py reads.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <map>
#include <set>

#include "audience_set_plan.h"

using namespace rwr;

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            ++failures;                                                      \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
        }                                                                    \
    } while (0)

// a call over n = 6 nodes with every argument right; the checks below break it one step at a time, from the last step up
struct Good {
    int64_t set_ptr[4] = {0, 2, 3, 6};
    int32_t set_idx[6] = {1, 4, 0, 5, 5, 2};
    double set_w[6] = {1.0, 0.25, 3.7, 0x1p-256, 0x1p256, 1.0};
    int32_t pool[3] = {5, 0, 5};
    int64_t deny_ptr[4] = {0, 0, 2, 2};
    int32_t deny_idx[2] = {3, 3};
    int64_t test_ptr[4] = {0, 1, 1, 3};
    int64_t test_ids[3] = {7, 8, 7};
    int64_t ids[3 * 4] = {}, pos[3] = {}, len[3] = {};
    double sc[3 * 4] = {};
    int32_t nodes[3 * 4] = {}, cnt[3] = {};
    AudCall call(AudDest dest) const
    {
        AudCall a;
        a.K = 3, a.set_ptr = set_ptr, a.set_idx = set_idx, a.set_w = set_w, a.n_iter = 3, a.cand_type = 1, a.etype_mask = 0x2u;
        a.exclude_members = 1, a.n_pool = 3, a.pool_idx = pool, a.deny_ptr = deny_ptr, a.deny_idx = deny_idx, a.dest = dest;
        a.out_score = const_cast<double *>(sc);
        if (dest == AUD_LISTS) {
            a.top_n = 4, a.out_id = const_cast<int64_t *>(ids), a.out_node = const_cast<int32_t *>(nodes);
            a.out_count = const_cast<int32_t *>(cnt);
        } else {
            a.test_ptr = test_ptr, a.test_ids = test_ids, a.out_pos = const_cast<int64_t *>(pos), a.out_len = const_cast<int64_t *>(len);
        }
        return a;
    }
};

static AudSetVerdict verdict(const AudCall &a, bool have = true) { return audience_set_check(a, have, 6).verdict; }

// Every step of the ladder, last to first: each fault is added to a call that already holds every LATER fault, and must win.
// Returns the faulty calls in ladder order for the "messages" mode.
struct Step {
    AudSetVerdict want;
    int32_t status;
    AudCall call;
    bool have_graph;
};

static std::vector<Step> ladder(AudDest dest, Good &g)
{
    static int64_t bad_test_ptr0[4] = {1, 1, 1, 3}, dec_test_ptr[4] = {0, 2, 1, 3};
    static int64_t big_test_ptr[4] = {0, 0, (int64_t)1 << 32, (int64_t)1 << 32};
    static int64_t bad_deny_ptr0[4] = {1, 1, 2, 2}, dec_deny_ptr[4] = {0, 2, 1, 2};
    static int32_t bad_deny_idx[2] = {3, 6}, bad_pool[3] = {5, -1, 9};
    static int64_t bad_ptr0[4] = {2, 2, 3, 6}, dec_ptr[4] = {0, 3, 2, 6}, empty_ptr[4] = {0, 2, 2, 5};
    static int32_t bad_idx[6] = {1, 4, 0, 6, 6, -2};   // (at the position of the first bad weight: the member is looked at first)
    static double bad_w[6] = {1.0, 0.25, 3.7, 0x1p-257, std::numeric_limits<double>::quiet_NaN(), -1.0};
    std::vector<Step> rev;
    AudCall a = g.call(dest);
    const bool lists = dest == AUD_LISTS;
    auto add = [&](AudSetVerdict v, int32_t st, bool have = true) {
        rev.push_back({v, st, a, have});
        const AudSetCheck c = audience_set_check(a, have, 6);
        CHECK(c.verdict == v);
        CHECK(audience_set_status("who", c, a, 6).status == st);
    };
    CHECK(verdict(a) == AUDSET_OK);
    CHECK(audience_set_status("who", audience_set_check(a, true, 6), a, 6).status == RWR_OK);
    if (!lists) {
        a.test_ptr = big_test_ptr; add(AUDSET_TEST_SET_TOO_LARGE, RWR_E_UNSUPPORTED);
        a.test_ids = nullptr; add(AUDSET_TEST_NULL_IDS, RWR_E_INVALID);
        a.test_ptr = dec_test_ptr; add(AUDSET_TEST_PTR_DECREASES, RWR_E_INVALID);
        a.test_ptr = bad_test_ptr0; add(AUDSET_TEST_BAD_PTR0, RWR_E_INVALID);
        a.out_pos = nullptr; add(AUDSET_TEST_NULL_OUT, RWR_E_INVALID);
        a.test_ptr = nullptr; add(AUDSET_TEST_NULL_PTR, RWR_E_INVALID);
    }
    a.deny_idx = bad_deny_idx; add(AUDSET_DENY_BAD_INDEX, RWR_E_RANGE);
    a.deny_idx = nullptr; add(AUDSET_DENY_NULL_IDX, RWR_E_INVALID);
    a.deny_ptr = dec_deny_ptr; add(AUDSET_DENY_PTR_DECREASES, RWR_E_INVALID);
    a.deny_ptr = bad_deny_ptr0; add(AUDSET_DENY_BAD_PTR0, RWR_E_INVALID);
    a.pool_idx = bad_pool; add(AUDSET_POOL_RANGE, RWR_E_RANGE);
    a.pool_idx = nullptr; add(AUDSET_NULL_POOL, RWR_E_INVALID);
    a.etype_mask = 0x100u; add(AUDSET_BAD_MASK, RWR_E_INVALID);
    a.cand_type = 256; add(AUDSET_BAD_CAND_TYPE, RWR_E_INVALID);
    a.n_iter = -1; add(AUDSET_NEGATIVE_ITER, RWR_E_INVALID);
    if (lists) { a.top_n = 1025; add(AUDSET_TOP_N_RANGE, RWR_E_RANGE); }
    a.set_w = bad_w; add(AUDSET_WEIGHT_RANGE, RWR_E_RANGE);
    a.set_idx = bad_idx; add(AUDSET_MEMBER_RANGE, RWR_E_RANGE);
    a.set_idx = nullptr; add(AUDSET_NULL_IDX, RWR_E_INVALID);
    a.set_ptr = empty_ptr; add(AUDSET_EMPTY_SET, RWR_E_INVALID);
    a.set_ptr = dec_ptr; add(AUDSET_PTR_DECREASES, RWR_E_INVALID);
    a.set_ptr = bad_ptr0; add(AUDSET_BAD_PTR0, RWR_E_INVALID);
    a.set_ptr = nullptr; add(AUDSET_NULL_ARG, RWR_E_INVALID);
    a.K = -1; add(AUDSET_NEGATIVE_K, RWR_E_INVALID);
    add(AUDSET_NULL_GRAPH, RWR_E_INVALID, false);
    return std::vector<Step>(rev.rbegin(), rev.rend());
}

static void check_ladder()
{
    Good g;
    for (AudDest dest : {AUD_LISTS, AUD_POSITIONS}) {
        const std::vector<Step> steps = ladder(dest, g);
        for (size_t j = 1; j < steps.size(); ++j) CHECK(steps[j].want > steps[j - 1].want);   // the enum is in ladder order
    }
    // what the refusals quote
    AudCall a = g.call(AUD_LISTS);
    int32_t idx[6] = {1, 4, 0, 5, 6, 2};
    a.set_idx = idx;
    AudSetCheck c = audience_set_check(a, true, 6);
    CHECK(c.verdict == AUDSET_MEMBER_RANGE && c.bad_k == 2 && c.bad_pos == 1 && c.bad_index == 6);
    CHECK(std::strstr(audience_set_status("E", c, a, 6).text, "E: member 6 (set 2, position 1) is outside [0, 6)"));
    a = g.call(AUD_LISTS);
    double w[6] = {1.0, std::numeric_limits<double>::infinity(), 3.7, 1.0, 1.0, 1.0};
    a.set_w = w;
    c = audience_set_check(a, true, 6);
    CHECK(c.verdict == AUDSET_WEIGHT_RANGE && c.bad_k == 0 && c.bad_pos == 1);
    CHECK(std::strstr(audience_set_status("E", c, a, 6).text, "(set 0, position 1)"));
    for (double bad : {0.0, -0.0, -1.0, 0x1p-257, 0x1.0000000000001p256, std::numeric_limits<double>::quiet_NaN(),
                       std::numeric_limits<double>::denorm_min()}) {
        w[1] = bad;
        CHECK(verdict(a) == AUDSET_WEIGHT_RANGE);
    }
    for (double ok : {0x1p-256, 0x1p256, 1.0, 3.7}) {
        w[1] = ok;
        CHECK(verdict(a) == AUDSET_OK);
    }
    a = g.call(AUD_LISTS);
    int64_t ep[4] = {0, 2, 2, 5};
    a.set_ptr = ep;
    c = audience_set_check(a, true, 6);
    CHECK(c.verdict == AUDSET_EMPTY_SET && c.bad_k == 1 && std::strstr(audience_set_status("E", c, a, 6).text, "set 1 is empty"));
    // the list tables are the lists entry's alone; top_n is not looked at by the positions entry
    a = g.call(AUD_LISTS);
    a.out_id = nullptr; CHECK(verdict(a) == AUDSET_NULL_ARG);
    a = g.call(AUD_LISTS);
    a.out_count = nullptr; CHECK(verdict(a) == AUDSET_NULL_ARG);
    a = g.call(AUD_LISTS);
    a.out_node = nullptr; CHECK(verdict(a) == AUDSET_OK);
    a.top_n = 0; CHECK(verdict(a) == AUDSET_TOP_N_RANGE);
    a = g.call(AUD_POSITIONS);
    a.top_n = 0, a.out_len = nullptr, a.out_score = nullptr; CHECK(verdict(a) == AUDSET_OK);
    // no weights, no pool (any negative count), an empty pool without an array, no deny lists
    a = g.call(AUD_LISTS);
    a.set_w = nullptr, a.n_pool = -7, a.pool_idx = nullptr, a.deny_ptr = nullptr, a.deny_idx = nullptr;
    CHECK(verdict(a) == AUDSET_OK);
    a.n_pool = 0; CHECK(verdict(a) == AUDSET_OK);
    // K == 0: no table is looked at, the other arguments still are (the no-op comes last, after the domain: api.hip)
    AudCall z;
    z.top_n = 5;
    CHECK(verdict(z) == AUDSET_OK);
    z.top_n = 0; CHECK(verdict(z) == AUDSET_TOP_N_RANGE);
    z.top_n = 5, z.n_iter = -2; CHECK(verdict(z) == AUDSET_NEGATIVE_ITER);
    z.n_iter = 0, z.dest = AUD_POSITIONS, z.top_n = 0; CHECK(verdict(z) == AUDSET_OK);
}

static void check_merge()
{
    // set 0: 4 listed three times, 1 once; set 1: node 4 again (one node in two sets), 0 twice
    const int64_t ptr[3] = {0, 5, 8};
    const int32_t idx[8] = {4, 1, 4, 9, 4, 0, 4, 0};
    const double w[8] = {0.1, 1.0, 0.2, 3.7, 0.3, 0.25, 3.7, 0.25};
    const AudSets m = aud_set_merge(2, ptr, idx, w);
    CHECK(m.ptr == (std::vector<int64_t>{0, 3, 5}) && m.idx == (std::vector<int32_t>{1, 4, 9, 0, 4}) && m.largest == 3);
    const double s4 = (0.1 + 0.2) + 0.3;                        // list order, from the first occurrence's weight on
    CHECK(m.w.size() == 5 && m.w[0] == 1.0 && m.w[1] == s4 && m.w[2] == 3.7 && m.w[3] == 0.5 && m.w[4] == 3.7);
    CHECK(0.1 + (0.2 + 0.3) != s4);                              // (the order matters for these three)
    const AudSets u = aud_set_merge(2, ptr, idx, nullptr);      // no weights: 1.0 per occurrence
    CHECK(u.idx == m.idx && u.w == (std::vector<double>{1.0, 3.0, 1.0, 2.0, 1.0}));
    // one-member unit sets: the targets themselves, the weight's bits kept
    const int64_t p1[4] = {0, 1, 2, 3};
    const int32_t t1[3] = {7, 2, 7};
    const AudSets o = aud_set_merge(3, p1, t1, nullptr);
    CHECK(o.ptr == (std::vector<int64_t>{0, 1, 2, 3}) && o.idx == (std::vector<int32_t>{7, 2, 7}) && o.largest == 1);
    CHECK(o.w == (std::vector<double>{1.0, 1.0, 1.0}));
    CHECK(aud_set_merge(0, nullptr, nullptr, nullptr).ptr == std::vector<int64_t>{0});
}

// brute force: cell (group, local slot, row) -> weight, from the merged sets and the slot assignment
static void check_pairs_and_targets()
{
    // 5 sets over 12 nodes; slots of 2 tiles x 2 (slots_per_group 4), so 7 slots form two groups with a padding slot each side
    const int64_t ptr[6] = {0, 3, 4, 6, 9, 10};
    const int32_t idx[10] = {3, 8, 3, 8, 5, 8, 3, 8, 3, 11};   // sets 0 and 3 are the same set {3, 8}; 8 is in sets 0, 1, 2, 3
    const double w[10] = {1.0, 0.25, 3.7, 1.0, 3.7, 0.25, 1.0, 0.25, 3.7, 1.0};
    const AudSets m = aud_set_merge(5, ptr, idx, w);
    const int32_t slot_k[8] = {2, -1, 0, 3, 1, 4, -1, -1};     // group 0: sets 2, 0, 3 (set 0 and its repeat); group 1: sets 1, 4
    for (size_t spg : {(size_t)4, (size_t)8, (size_t)2}) {
        const AudSetPairs p = aud_set_pairs(m, 8, slot_k, spg);
        const size_t ngroups = (8 + spg - 1) / spg;
        CHECK(p.group_off.size() == ngroups + 1 && p.group_off[0] == 0 && (size_t)p.group_off.back() == p.slot.size());
        CHECK(p.slot.size() == p.row.size() && p.row.size() == p.w.size());
        std::map<std::pair<size_t, std::pair<int32_t, int32_t>>, double> want, got;
        for (size_t q = 0; q < 8; ++q)
            if (slot_k[q] >= 0)
                for (int64_t j = m.ptr[slot_k[q]]; j < m.ptr[slot_k[q] + 1]; ++j)
                    want[{q / spg, {(int32_t)(q % spg), m.idx[j]}}] = m.w[j];
        for (size_t gi = 0; gi < ngroups; ++gi)
            for (int64_t j = p.group_off[gi]; j < p.group_off[gi + 1]; ++j) {
                CHECK(p.slot[j] >= 0 && (size_t)p.slot[j] < spg);
                CHECK(got.emplace(std::make_pair(gi, std::make_pair(p.slot[j], p.row[j])), p.w[j]).second);   // a cell occurs once
            }
        CHECK(got == want);
        // the exclusion tables: per group, node -> the set of local slots whose set holds it
        const AudTargets t = aud_set_targets(m, 8, slot_k, spg);
        CHECK(t.group_off.size() == ngroups + 1 && t.ptr.size() == t.node.size() + 1 && (size_t)t.ptr.back() == t.slot.size());
        for (size_t gi = 0; gi < ngroups; ++gi) {
            std::map<int32_t, std::set<int32_t>> wt;
            for (const auto &cell : want)
                if (cell.first.first == gi) wt[cell.first.second.second].insert(cell.first.second.first);
            const int64_t e0 = t.group_off[gi], e1 = t.group_off[gi + 1];
            CHECK((size_t)(e1 - e0) == wt.size());
            for (int64_t e = e0; e < e1; ++e) {
                CHECK(e == e0 || t.node[e] > t.node[e - 1]);                      // distinct, ascending: aud_target_find searches it
                std::set<int32_t> slots(t.slot.begin() + t.ptr[e], t.slot.begin() + t.ptr[e + 1]);
                CHECK((int32_t)slots.size() == t.ptr[e + 1] - t.ptr[e]);         // no slot twice
                CHECK(wt.count(t.node[e]) && wt[t.node[e]] == slots);
                for (int32_t a = t.ptr[e]; a + 1 < t.ptr[e + 1]; ++a) CHECK(t.slot[a] < t.slot[a + 1]);
                CHECK(aud_target_find(t.node.data() + e0, (int32_t)(e1 - e0), t.node[e]) == (int32_t)(e - e0));
            }
        }
        if (spg == 4) {
            // group 0 holds sets 2 = {5, 8}, 0 = {3, 8} and 3 = {3, 8}: node 8, a member shared by three sets (two of them one
            // set that repeats), owns slots 0, 2, 3; node 3 owns slots 2 and 3 -- so a source that links to both members of
            // set 0 finds slot 2 under either of them and marks the one cell twice; node 5 owns slot 0 alone
            CHECK(t.group_off[1] == 3 && t.node[0] == 3 && t.node[1] == 5 && t.node[2] == 8);
            CHECK(std::vector<int32_t>(t.slot.begin() + t.ptr[2], t.slot.begin() + t.ptr[3]) == (std::vector<int32_t>{0, 2, 3}));
            CHECK(std::vector<int32_t>(t.slot.begin() + t.ptr[0], t.slot.begin() + t.ptr[1]) == (std::vector<int32_t>{2, 3}));
            // the merged weights of the repeated members: 3 -> (1.0 + 3.7), in both slots of the set that repeats
            CHECK((want[{0, {2, 3}}] == 1.0 + 3.7) && (want[{0, {3, 3}}] == 1.0 + 3.7) && (want[{0, {2, 8}}] == 0.25));
            // across the group boundary: set 1 = {8} sits in group 1, local slot 0
            CHECK((want[{1, {0, 8}}] == 1.0) && (want[{1, {1, 11}}] == 1.0) && p.group_off[1] == 6 && p.group_off[2] == 8);
        }
    }
    // one-member sets: the tables are aud_targets() of the slots' targets, entry for entry
    const int64_t p1[6] = {0, 1, 2, 3, 4, 5};
    const int32_t t1[5] = {7, 2, 7, 0, 2};
    const AudSets o = aud_set_merge(5, p1, t1, nullptr);
    const int32_t sk[6] = {4, 0, -1, 2, 1, 3};
    int32_t slot_target[6];
    for (int q = 0; q < 6; ++q) slot_target[q] = sk[q] >= 0 ? t1[sk[q]] : -1;
    for (size_t spg : {(size_t)2, (size_t)4, (size_t)6}) {
        const AudTargets a = aud_targets(6, slot_target, spg), b = aud_set_targets(o, 6, sk, spg);
        CHECK(a.group_off == b.group_off && a.node == b.node && a.ptr == b.ptr && a.slot == b.slot);
    }
}

static int print_messages()
{
    Good g;
    for (AudDest dest : {AUD_LISTS, AUD_POSITIONS}) {
        const char *who = dest == AUD_LISTS ? "rwr_recommend_audience_set_batch" : "rwr_recommend_audience_set_positions_batch";
        for (const Step &s : ladder(dest, g)) {
            const AudStatus st = audience_set_status(who, audience_set_check(s.call, s.have_graph, 6), s.call, 6);
            std::printf("%d %d %s\n", (int)s.want, (int)st.status, st.text);
        }
    }
    return failures;
}

int main(int argc, char **argv)
{
    if (argc > 1 && !std::strcmp(argv[1], "messages")) return print_messages();
    check_ladder();
    check_merge();
    check_pairs_and_targets();
    std::printf("%d failures\n", failures);
    return failures != 0;
}
