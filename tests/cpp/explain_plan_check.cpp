// Host-side check of the explained entry's plan (recommendersystems_amd/csrc/explain_plan.h), built against the header alone
// by tests/test_explain_plan.py: the addend's two roundings, the selection model against a brute-force sort for every n_why
// and lane count, why_total, and the table geometry.  (The argument verdicts: tests/cpp/typed_call_check.cpp.)  Prints every
// failure and exits non-zero if there is one.
#include "explain_plan.h"

#include <algorithm>
#include <cmath>
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

// ---- the addend ----------------------------------------------------------------------------------------------------------------

static void check_addend()
{
    // two roundings: c1 * y is rounded before the weight multiplies it (a fused or re-associated form differs on these)
    std::mt19937_64 rng(11);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    int differs = 0;
    for (int i = 0; i < 2000; ++i) {
        const double c1 = 1.0 - (double)(float)u(rng), y = u(rng) * 1000.0, w = u(rng);
        volatile double rw = c1 * y;
        volatile double want = rw * w;
        if (why_bits(why_addend(c1, y, w)) != why_bits(want)) fail("addend: not the two separately rounded products");
        volatile double other = c1 * (y * w);
        differs += why_bits(other) != why_bits(want);
    }
    if (differs == 0) fail("addend: the sample cannot tell the association apart");
    if (why_is_reason(0.0) || why_is_reason(-0.0) || why_is_reason(std::nan("")) || !why_is_reason(5e-324)) fail("is_reason");
    if (why_value(why_bits(0.1)) != 0.1) fail("bits round trip");
    // positive doubles order as their bit patterns
    const double ds[] = {5e-324, 1e-300, 0.5, 1.0, 1.0000000000000002, 3.0, 1e300};
    for (size_t i = 1; i < sizeof ds / sizeof ds[0]; ++i)
        if (!(why_bits(ds[i]) > why_bits(ds[i - 1]))) fail("bit order of positive doubles");
}

// ---- the selection ---------------------------------------------------------------------------------------------------------------

struct Ref {
    std::vector<uint32_t> pos;
    std::vector<uint64_t> bits;
    int64_t total;
};

static Ref brute(const std::vector<double> &y, const std::vector<double> &w, double c1, int32_t r)
{
    std::vector<std::pair<uint64_t, uint32_t>> all;
    for (size_t e = 0; e < y.size(); ++e) {
        volatile double rw = c1 * y[e];
        volatile double a = rw * w[e];
        if (a > 0.0) all.push_back({why_bits(a), (uint32_t)e});
    }
    std::sort(all.begin(), all.end(), [](const auto &a, const auto &b) { return a.first != b.first ? a.first > b.first : a.second < b.second; });
    Ref ref;
    ref.total = (int64_t)all.size();
    for (int32_t i = 0; i < r; ++i) {
        ref.pos.push_back((size_t)i < all.size() ? all[(size_t)i].second : ~0u);
        ref.bits.push_back((size_t)i < all.size() ? all[(size_t)i].first : 0);
    }
    return ref;
}

static void check_select()
{
    std::mt19937 rng(3);
    const int64_t degs[] = {0, 1, 2, 3, 7, 8, 9, 63, 64, 65, 255, 256, 257, 513, 700};
    const int32_t lanes[] = {1, 2, 64, 256};
    for (int64_t deg : degs)
        for (int style = 0; style < 4; ++style) {
            std::vector<double> y((size_t)deg), w((size_t)deg);
            for (int64_t e = 0; e < deg; ++e) {
                // 0: all distinct; 1: few values, ties everywhere; 2: mostly zero sources; 3: all equal
                const double v = style == 0 ? (double)(rng() % 100000 + 1) / 7.0 : style == 1 ? (double)(rng() % 3 + 1) : style == 2 ? (rng() % 5 ? 0.0 : (double)(rng() % 4)) : 2.5;
                y[(size_t)e] = v;
                w[(size_t)e] = style == 0 ? 1.0 / (double)(rng() % 50 + 1) : 0.125;
            }
            for (int32_t r = 0; r <= WHY_MAX; ++r) {
                const Ref ref = brute(y, w, 0.85, r);
                for (int32_t ln : lanes) {
                    std::vector<uint32_t> pos((size_t)r + 1, 7u);
                    std::vector<uint64_t> bits((size_t)r + 1, 7u);
                    const int64_t total = why_select(deg, 0.85, [&](int64_t e) { return y[(size_t)e]; }, [&](int64_t e) { return w[(size_t)e]; }, r, ln,
                                                     pos.data(), bits.data());
                    const std::string at = "deg " + std::to_string(deg) + " style " + std::to_string(style) + " r " + std::to_string(r) + " lanes " + std::to_string(ln);
                    if (total != ref.total) fail("why_total at " + at);
                    for (int32_t i = 0; i < r; ++i)
                        if (pos[(size_t)i] != ref.pos[(size_t)i] || bits[(size_t)i] != ref.bits[(size_t)i]) { fail("selection at " + at); break; }
                    if (pos[(size_t)r] != 7u || bits[(size_t)r] != 7u) fail("selection writes behind its r cells at " + at);
                }
            }
        }
    // a list: sentinels in front, merge ignores sentinels and empties, equal keys of different positions keep position order
    WhyList a, b;
    why_list_init(a, 2), why_list_init(b, 2);
    for (int j = 0; j < WHY_MAX - 2; ++j)
        if (!why_is_top(a.k[j])) fail("list init: sentinel");
    if (!why_is_empty(a.k[WHY_MAX - 1]) || !why_is_empty(a.k[WHY_MAX - 2])) fail("list init: empty");
    why_list_insert(a, WhyKey{why_bits(1.0), 9}), why_list_insert(b, WhyKey{why_bits(1.0), 4}), why_list_insert(b, WhyKey{why_bits(1.0), 12});
    why_list_merge(a, b);
    if (a.k[WHY_MAX - 2].pos != 4 || a.k[WHY_MAX - 1].pos != 9) fail("merge: equal values by position");
    for (int j = 0; j < WHY_MAX - 2; ++j)
        if (!why_is_top(a.k[j])) fail("merge: a sentinel moved");
}

// ---- the tables ------------------------------------------------------------------------------------------------------------------

static void check_tables()
{
    if (why_entry_cells(3, 5) != 15 || why_reason_cells(3, 5, 8) != 120 || why_reason_cells(3, 5, 0) != 0) fail("table sizes");
    if (why_entry_cells(0x7FFFFFFF, 1024) != (size_t)0x7FFFFFFF * 1024) fail("table sizes: 64-bit");
    if (why_offset(0, 0, 5, 3) != 0 || why_offset(2, 4, 5, 3) != 42 || why_offset(1, 0, 5, 3) != 15) fail("offsets");
    if (why_offset(0x7FFFFFFF, 1023, 1024, 8) != ((size_t)0x7FFFFFFF * 1024 + 1023) * 8) fail("offsets: 64-bit");
}

int main()
{
    check_addend();
    check_select();
    check_tables();
    std::printf("%d failures\n", failures);
    return failures != 0;
}
