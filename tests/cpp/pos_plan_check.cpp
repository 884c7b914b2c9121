// Host-side check of the positions plan (recommendersystems_amd/csrc/pos_plan.h), built against the headers alone by
// tests/test_pos_plan.py: where the answer of every caller entry lies in the device result arrays, against a direct restatement
// (std::set per slot, the entry's place counted in it) over hand-made and random slot assignments -- padding slots, several
// tile groups, the same set at two batch positions (duplicate seeds sit in different slots), a batch position that two slots
// hold and one that no slot holds, empty sets, duplicate and absent ids; then the scatter of made-up device arrays back into
// the caller's order.  Prints every failure and exits non-zero if there is one.
#include "pos_plan.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <iterator>
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

static void check_case(const std::string &name, const Sets &sets, const std::vector<int32_t> &slot_k, size_t per_group)
{
    const int32_t K = (int32_t)sets.size();
    const size_t nslots = slot_k.size();
    std::vector<int64_t> ptr(1, 0), ids;
    for (const auto &s : sets) {
        ids.insert(ids.end(), s.begin(), s.end());
        ptr.push_back((int64_t)ids.size());
    }
    int64_t out = 0;
    const EvalPlan ev = eval_plan(nslots, slot_k.data(), per_group, K, ptr.data(), ids.empty() ? nullptr : ids.data(), &out, &out);
    if (K > 0 && ev.check.verdict != EVAL_OK) { fail(name + ": the evaluation plan's verdict"); return; }
    const PosPlan p = pos_plan(ev, nslots, slot_k.data(), K, ptr.data(), ids.data());
    if (K <= 0) {
        if (!p.entry_u.empty() || p.n_pos || p.n_score || p.n_len) fail(name + ": K = 0 plans something");
        return;
    }
    if (p.n_pos != ev.ids.size() || p.n_score != ev.ids.size() || p.n_len != (size_t)K) fail(name + ": result array sizes");
    if (p.entry_u.size() != ids.size() || p.slot_of_k.size() != (size_t)K) { fail(name + ": plan sizes"); return; }
    // the direct restatement: the first slot that holds k; in it the ids of set k, ascending and once each; the entry's place
    for (int32_t k = 0; k < K; ++k) {
        int64_t slot = -1;
        for (size_t q = 0; q < nslots && slot < 0; ++q)
            if (slot_k[q] == k) slot = (int64_t)q;
        if (p.slot_of_k[(size_t)k] != slot) fail(name + ": slot of batch position " + std::to_string(k));
        const std::set<int64_t> want(sets[(size_t)k].begin(), sets[(size_t)k].end());
        for (int64_t j = ptr[(size_t)k]; j < ptr[(size_t)k + 1]; ++j) {
            const int64_t u = p.entry_u[(size_t)j];
            if (slot < 0) {
                if (u != -1) fail(name + ": an entry of a batch position without a slot has a place");
                continue;
            }
            const int64_t place = ev.slot_off[(size_t)slot] + (int64_t)std::distance(want.begin(), want.find(ids[(size_t)j]));
            if (u != place) fail(name + ": entry " + std::to_string(j) + " of set " + std::to_string(k));
            else if (u < ev.slot_off[(size_t)slot] || u >= ev.slot_off[(size_t)slot + 1] || ev.ids[(size_t)u] != ids[(size_t)j])
                fail(name + ": entry " + std::to_string(j) + " does not point at its id in its slot");
        }
    }
    // the scatter: device arrays that name their own index; a "no hit" keeps -1 and gets +0.0 whatever the score array holds
    std::vector<int64_t> dpos(ev.ids.size()), dlen((size_t)K);
    std::vector<double> dsc(ev.ids.size());
    for (size_t u = 0; u < dpos.size(); ++u) {
        dpos[u] = u % 3 == 2 ? -1 : (int64_t)(1000 + u);
        dsc[u] = u % 3 == 2 ? 7.5 : 0.25 * (double)u;
    }
    for (int32_t k = 0; k < K; ++k) dlen[(size_t)k] = 50 + k;
    std::vector<int64_t> pos(ids.size() + 1, -99), len((size_t)K + 1, -99);
    std::vector<double> sc(ids.size() + 1, -99.0);
    pos_scatter(p, K, dpos.data(), dsc.data(), dlen.data(), pos.data(), sc.data(), len.data());
    if (pos.back() != -99 || sc.back() != -99.0 || len.back() != -99) fail(name + ": the scatter writes past its arrays");
    for (size_t j = 0; j < ids.size(); ++j) {
        const int64_t u = p.entry_u[j];
        const int64_t wp = u < 0 ? -1 : dpos[(size_t)u];
        const double ws = wp < 0 ? 0.0 : dsc[(size_t)u];
        if (pos[j] != wp || std::memcmp(&sc[j], &ws, 8) != 0) fail(name + ": scattered entry " + std::to_string(j));
    }
    for (int32_t k = 0; k < K; ++k)
        if (len[(size_t)k] != 50 + k) fail(name + ": scattered length " + std::to_string(k));
    // duplicates of one id within a set share their place; NULL score_out and list_len are legal
    for (int32_t k = 0; k < K; ++k)
        for (int64_t a = ptr[(size_t)k]; a < ptr[(size_t)k + 1]; ++a)
            for (int64_t b = a + 1; b < ptr[(size_t)k + 1]; ++b)
                if (p.slot_of_k[(size_t)k] >= 0 && (ids[(size_t)a] == ids[(size_t)b]) != (p.entry_u[(size_t)a] == p.entry_u[(size_t)b]))
                    fail(name + ": duplicates of set " + std::to_string(k));
    pos_scatter(p, K, dpos.data(), dsc.data(), dlen.data(), pos.data(), nullptr, nullptr);
}

// the driver's dealing: vector k in slot (k % ntiles) * G + k / ntiles, the rest padding
static std::vector<int32_t> dealt(int32_t K, int G)
{
    const size_t ntiles = ((size_t)K + G - 1) / G;
    std::vector<int32_t> slot_k(ntiles * G, -1);
    for (int32_t k = 0; k < K; ++k) slot_k[(size_t)(k % ntiles) * G + (size_t)(k / ntiles)] = k;
    return slot_k;
}

int main()
{
    check_case("K = 0", {}, {}, 1);
    check_case("one empty set", {{}}, dealt(1, 1), 1);
    check_case("duplicates", {{5, 5, 2, 5, 2, 9}}, dealt(1, 4), 4);
    check_case("extremes", {{INT64_MAX, INT64_MIN, 0, -1, INT64_MAX}}, dealt(1, 2), 2);
    // the same seed twice with different sets, and twice with the same set: two slots, two ranges
    check_case("duplicate seeds", {{3, 1}, {1, 3, 3, 7}, {3, 1}, {}}, dealt(4, 2), 2);
    check_case("two groups of two tiles", {{3}, {6, 3}, {2}, {3, 3}, {4}, {6}, {}, {0}, {8, 8}}, dealt(9, 2), 4);
    // the restart fallback: one slot per batch position, every slot its own group
    check_case("one group per vector", {{4, 4}, {}, {9, 1, 4}}, {0, 1, 2}, 1);
    // a batch position in two slots (the first answers), one in no slot (no answer), slots in any order
    check_case("two slots hold position 1", {{1, 2}, {2, 2, 5}, {7}}, {2, -1, 1, 0, 1, -1}, 2);
    check_case("no slot holds position 0", {{1, 2}, {5}}, {-1, 1, -1, -1}, 4);

    std::mt19937_64 rng(23);
    for (int it = 0; it < 600; ++it) {
        const int K = 1 + (int)(rng() % 12);
        Sets sets((size_t)K);
        for (auto &s : sets) {
            const int len = (int)(rng() % 9);
            for (int j = 0; j < len; ++j) s.push_back((int64_t)(rng() % 12) - 3);
        }
        if (K > 2 && it % 3 == 0) sets[(size_t)K - 1] = sets[0];           // a duplicate seed's set
        const int G = 1 << (rng() % 7), TG = 1 + (int)(rng() % 3);
        std::vector<int32_t> slot_k = dealt(K, G);
        if (it % 2) {                                                        // any assignment: shuffled, some positions dropped or doubled
            std::shuffle(slot_k.begin(), slot_k.end(), rng);
            for (auto &k : slot_k)
                if (rng() % 7 == 0) k = rng() % 2 ? -1 : (int32_t)(rng() % K);
        }
        check_case("random " + std::to_string(it), sets, slot_k, (size_t)TG * G);
    }

    // a plan whose sets failed their check plans nothing
    {
        const int64_t bad_ptr[3] = {0, 2, 1}, ids[2] = {1, 2};
        const int32_t slot_k[2] = {0, 1};
        int64_t out = 0;
        const EvalPlan ev = eval_plan(2, slot_k, 2, 2, bad_ptr, ids, &out, &out);
        const PosPlan p = pos_plan(ev, 2, slot_k, 2, bad_ptr, ids);
        if (ev.check.verdict != EVAL_PTR_DECREASES || !p.entry_u.empty() || p.n_pos || p.n_len) fail("refused sets plan something");
        const EvalPlan no_out = eval_plan(2, slot_k, 2, 2, bad_ptr, ids, nullptr, nullptr);
        if (no_out.check.verdict != EVAL_NULL_OUT) fail("a NULL pos_out is not the first verdict");
    }
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
