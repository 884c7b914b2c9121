// Host-side check of the node append plan (recommendersystems_amd/csrc/node_append_plan.h), built against the headers alone by
// tests/test_node_append_plan.py: the merge positions of the ITEM order against std::stable_sort over the grown id set (the
// order rwr_graph_create's stable radix sort produces: ids descending, equal ids in row-ascending order), the sort of the new
// ITEM rows, the id key range, and the grown row pointers -- with and without links in the same call -- against a brute-force
// list-of-lists rebuild.  Prints every failure and exits non-zero if there is one.
#include "append_plan.h"
#include "node_append_plan.h"

#include <algorithm>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

using namespace rwr;

static int failures = 0;
static long cases_checked = 0;

static void fail(const std::string &what)
{
    if (++failures <= 40) std::printf("FAIL %s\n", what.c_str());
}

constexpr uint8_t ITEM = 1, USER = 0, ETC = 2;

// old nodes (ids, types), new nodes (ids, types): the merged item_order and item_rows against a sort of everything
static void check_case(const std::string &name, const std::vector<int64_t> &old_id, const std::vector<uint8_t> &old_type,
                       const std::vector<int64_t> &new_id, const std::vector<uint8_t> &new_type)
{
    ++cases_checked;
    const int32_t n_old = (int32_t)old_id.size(), n_new = (int32_t)new_id.size(), n = n_old + n_new;
    std::vector<int64_t> id(old_id);
    id.insert(id.end(), new_id.begin(), new_id.end());
    std::vector<uint8_t> type(old_type);
    type.insert(type.end(), new_type.begin(), new_type.end());

    // what create builds: ITEM rows ascending, then stably by id descending
    auto orders = [&](int32_t upto, std::vector<int32_t> &rows, std::vector<int32_t> &order) {
        rows.clear();
        for (int32_t i = 0; i < upto; ++i)
            if (type[(size_t)i] == ITEM) rows.push_back(i);
        order = rows;
        std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return id[(size_t)a] > id[(size_t)b]; });
    };
    std::vector<int32_t> rows_old, A, rows_want, want;
    orders(n_old, rows_old, A);
    orders(n, rows_want, want);

    const NodeAppendPlan p = node_append_plan(n_old, n_new, new_id.data(), new_type.data(), ITEM);
    if (p.verdict != NODE_APPEND_OK) { fail(name + ": verdict"); return; }
    if (p.n_old != n_old || p.n_total != n) fail(name + ": n_old / n_total");
    const int32_t no = (int32_t)A.size(), nn = p.n_new_items;
    if (no + nn != (int32_t)want.size()) { fail(name + ": item count"); return; }
    if ((int32_t)p.new_item_rows.size() != nn || (int32_t)p.new_item_sorted.size() != nn) { fail(name + ": table lengths"); return; }

    // item_rows: the resident rows, then the new ones
    std::vector<int32_t> rows_got(rows_old);
    rows_got.insert(rows_got.end(), p.new_item_rows.begin(), p.new_item_rows.end());
    if (rows_got != rows_want) fail(name + ": item_rows");

    // B against a stable sort of the new rows
    std::vector<int32_t> B_want(p.new_item_rows);
    std::stable_sort(B_want.begin(), B_want.end(), [&](int32_t a, int32_t b) { return id[(size_t)a] > id[(size_t)b]; });
    if (p.new_item_sorted != B_want) fail(name + ": new ITEM rows by id");
    const std::vector<int32_t> &B = p.new_item_sorted;

    // the merge: every destination in range, written once, and the result is create's order
    std::vector<int32_t> got((size_t)(no + nn), -1);
    std::vector<int> hit((size_t)(no + nn), 0);
    auto put = [&](int32_t to, int32_t row) {
        if (to < 0 || to >= no + nn) { fail(name + ": destination " + std::to_string(to) + " out of range"); return; }
        ++hit[(size_t)to];
        got[(size_t)to] = row;
    };
    for (int32_t q = 0; q < no; ++q)
        put(nap_old_dest(q, id[(size_t)A[(size_t)q]], nn, [&](int32_t r) { return id[(size_t)B[(size_t)r]]; }), A[(size_t)q]);
    for (int32_t r = 0; r < nn; ++r)
        put(nap_new_dest(r, id[(size_t)B[(size_t)r]], no, [&](int32_t q) { return id[(size_t)A[(size_t)q]]; }), B[(size_t)r]);
    for (int32_t t = 0; t < no + nn; ++t)
        if (hit[(size_t)t] != 1) { fail(name + ": position " + std::to_string(t) + " written " + std::to_string(hit[(size_t)t]) + " times"); break; }
    if (got != want) fail(name + ": merged item_order differs from the stable sort");

    // the id key range of the grown set, as create computes it from all ITEM ids
    if (nn > 0) {
        uint64_t lo = ~0ull, hi = 0;
        for (int32_t i = n_old; i < n; ++i)
            if (type[(size_t)i] == ITEM) { lo = std::min(lo, nap_orderable(id[(size_t)i])); hi = std::max(hi, nap_orderable(id[(size_t)i])); }
        if (p.key_lo != lo || p.key_hi != hi) fail(name + ": key range of the new items");
    }
}

static std::vector<uint8_t> all_items(size_t k) { return std::vector<uint8_t>(k, ITEM); }

static void named_cases()
{
    check_case("all ids equal", {5, 5, 5, 5}, all_items(4), {5, 5, 5}, all_items(3));
    check_case("new below", {10, 30, 20}, all_items(3), {1, 2, 0}, all_items(3));
    check_case("new above", {10, 30, 20}, all_items(3), {31, 99, 32}, all_items(3));
    check_case("new inside", {10, 30, 20}, all_items(3), {11, 29, 25, 15}, all_items(4));
    check_case("new equal to old", {10, 30, 20}, all_items(3), {30, 10, 20, 20}, all_items(4));
    check_case("negative ids", {-5, 3, 0, -100}, all_items(4), {-6, -5, -1, 4, INT64_MIN, INT64_MAX}, all_items(6));
    check_case("old at the extremes", {INT64_MIN, INT64_MAX}, all_items(2), {0, INT64_MIN, INT64_MAX, -1}, all_items(4));
    check_case("no old items", {7, 8}, {USER, ETC}, {3, 9, 3}, all_items(3));
    check_case("no old nodes' items, no new items", {7, 8}, {USER, ETC}, {3, 9}, {USER, USER});
    check_case("no new items", {7, 8, 9}, all_items(3), {3, 9}, {USER, ETC});
    check_case("no new nodes", {7, 8, 9}, {ITEM, USER, ITEM}, {}, {});
    check_case("mixed types", {7, 8, 9, 7}, {ITEM, USER, ITEM, ITEM}, {8, 7, 7, 100, -3}, {ITEM, ITEM, USER, ETC, ITEM});
    {   // 1 old x 1000 new and the reverse, ids colliding with the one
        std::vector<int64_t> many(1000);
        for (int i = 0; i < 1000; ++i) many[(size_t)i] = (int64_t)((i * 7919) % 41) - 20;
        check_case("1 old x 1000 new", {3}, all_items(1), many, all_items(1000));
        check_case("1000 old x 1 new", many, all_items(1000), {3}, all_items(1));
        check_case("1000 old x 1 new below all", many, all_items(1000), {-21}, all_items(1));
        check_case("1000 old x 1 new above all", many, all_items(1000), {21}, all_items(1));
    }
}

static void random_cases()
{
    std::mt19937_64 rng(20241019);
    for (int c = 0; c < 800; ++c) {
        const int style = c % 8;
        const int32_t n_old = (int32_t)(rng() % 60), n_new = (int32_t)(rng() % 60);
        // few distinct ids (many ties), a narrow range, the full 64-bit range, a range around zero
        auto draw = [&]() -> int64_t {
            switch (style) {
                case 0: return (int64_t)(rng() % 4);
                case 1: return (int64_t)(rng() % 50) - 25;
                case 2: return (int64_t)rng();
                case 3: return (int64_t)(rng() % 3) - 1;
                case 4: return (int64_t)(rng() % 100000) + 500;
                case 5: return (rng() & 1) ? INT64_MIN + (int64_t)(rng() % 3) : INT64_MAX - (int64_t)(rng() % 3);
                case 6: return (int64_t)(rng() % 2049) << 11;          // digits of the radix passes
                default: return (int64_t)(rng() % 1000) - 500;
            }
        };
        std::vector<int64_t> oi((size_t)n_old), ni((size_t)n_new);
        std::vector<uint8_t> ot((size_t)n_old), nt((size_t)n_new);
        for (int32_t i = 0; i < n_old; ++i) { oi[(size_t)i] = draw(); ot[(size_t)i] = (uint8_t)(rng() % 3 == 0 ? USER : ITEM); }
        for (int32_t i = 0; i < n_new; ++i) { ni[(size_t)i] = draw(); nt[(size_t)i] = (uint8_t)(rng() % 4 == 0 ? ETC : ITEM); }
        check_case("random " + std::to_string(c) + " (style " + std::to_string(style) + ")", oi, ot, ni, nt);
    }
    // the sort of the new rows over two and three radix passes
    for (const int64_t span : {(int64_t)2047, (int64_t)2048, (int64_t)5000000, (int64_t)1 << 40}) {
        std::vector<int64_t> ni(3000);
        for (auto &v : ni) v = (int64_t)(rng() % (uint64_t)span) - span / 2;
        check_case("wide span " + std::to_string(span), {0, span, -span}, all_items(3), ni, all_items(3000));
    }
}

// the grown row pointers: lists of lists with empty new rows, the links of the call appended, flattened again
static void rowptr_cases()
{
    std::mt19937_64 rng(4242);
    for (int c = 0; c < 300; ++c) {
        ++cases_checked;
        const std::string name = "rowptr " + std::to_string(c);
        const int32_t n_old = 1 + (int32_t)(rng() % 30), n_new = (int32_t)(rng() % 20), n = n_old + n_new;
        std::vector<int64_t> rp((size_t)n_old + 1, 0);
        for (int32_t i = 0; i < n_old; ++i) rp[(size_t)i + 1] = rp[(size_t)i] + (int64_t)(rng() % 3 == 0 ? 0 : rng() % 5);
        const int64_t count = c % 5 == 0 ? 0 : (int64_t)(rng() % 50);
        std::vector<int32_t> src((size_t)count), dst((size_t)count);
        for (int64_t q = 0; q < count; ++q) {
            // (a third of the links leave a new node, when there is one)
            src[(size_t)q] = (n_new > 0 && rng() % 3 == 0) ? n_old + (int32_t)(rng() % (uint64_t)n_new) : (int32_t)(rng() % (uint64_t)n);
            dst[(size_t)q] = (int32_t)(rng() % (uint64_t)n);
        }
        // brute force
        std::vector<int64_t> len((size_t)n, 0);
        for (int32_t i = 0; i < n_old; ++i) len[(size_t)i] = rp[(size_t)i + 1] - rp[(size_t)i];
        for (int64_t q = 0; q < count; ++q) ++len[(size_t)src[(size_t)q]];
        std::vector<int64_t> want((size_t)n + 1, 0);
        for (int32_t i = 0; i < n; ++i) want[(size_t)i + 1] = want[(size_t)i] + len[(size_t)i];

        std::vector<int64_t> got(rp);
        got.shrink_to_fit();           // (so that the growth reallocates: the sanitizer then sees every stale access)
        node_append_extend_rowptr(got, n_old, n);
        if ((int32_t)got.size() != n + 1) { fail(name + ": extended length"); continue; }
        for (int32_t i = n_old; i <= n; ++i)
            if (got[(size_t)i] != rp[(size_t)n_old]) { fail(name + ": extended entry " + std::to_string(i)); break; }
        const AppendPlan plan = append_plan(n, got.data(), count, src.data(), dst.data());
        if (plan.verdict != APPEND_OK) { fail(name + ": verdict"); continue; }
        // what k_append_rowptr computes per entry ...
        for (int32_t i = 0; i <= n; ++i)
            if (rp[(size_t)(i < n_old ? i : n_old)] + plan.row_shift(i) != want[(size_t)i]) { fail(name + ": device row pointer " + std::to_string(i)); break; }
        // ... and the host's running update
        node_append_shift_rowptr(got, n, plan.srcs, plan.cum);
        if (got != want) fail(name + ": host row pointers");
        // a link leaving a new node lands inside that node's new row
        for (int64_t q = 0; q < count; ++q) {
            const int64_t f = plan.new_index[(size_t)q];
            if (f < want[(size_t)src[(size_t)q]] || f >= want[(size_t)src[(size_t)q] + 1]) { fail(name + ": link " + std::to_string(q) + " outside its row"); break; }
        }
        // the range check uses the NEW bound
        if (count > 0) {
            std::vector<int32_t> bad(src);
            bad[0] = n;
            got.assign(rp.begin(), rp.end());
            node_append_extend_rowptr(got, n_old, n);
            if (append_plan(n, got.data(), count, bad.data(), dst.data()).verdict != APPEND_BAD_SRC) fail(name + ": src == n_total accepted");
            bad = dst;
            bad[0] = n;
            if (append_plan(n, got.data(), count, src.data(), bad.data()).verdict != APPEND_BAD_DST) fail(name + ": dst == n_total accepted");
        }
    }
}

static void limits()
{
    ++cases_checked;
    const int64_t one_id = 1;
    const uint8_t one_type = ITEM;
    if (node_append_plan(INT32_MAX, 1, &one_id, &one_type, ITEM).verdict != NODE_APPEND_TOO_MANY) fail("INT32_MAX + 1 nodes accepted");
    if (node_append_plan(INT32_MAX, 0, nullptr, nullptr, ITEM).verdict != NODE_APPEND_OK) fail("n_new == 0 at INT32_MAX refused");
    if (node_append_plan(INT32_MAX - 1, 1, &one_id, &one_type, ITEM).verdict != NODE_APPEND_OK) fail("INT32_MAX nodes refused");
    // create's key parameters: top = the largest id, bits of the range, at least one
    uint64_t top = 7;
    int32_t bits = 7;
    node_append_id_keys(false, 5, 9, &top, &bits);
    if (top != 0 || bits != 1) fail("id keys without an item");
    node_append_id_keys(true, 9, 9, &top, &bits);
    if (top != 9 || bits != 1) fail("id keys of one id");
    node_append_id_keys(true, nap_orderable(-3), nap_orderable(12), &top, &bits);
    if (top != nap_orderable(12) || bits != 4) fail("id keys of [-3, 12]");
    node_append_id_keys(true, nap_orderable(INT64_MIN), nap_orderable(INT64_MAX), &top, &bits);
    if (top != ~0ull || bits != 64) fail("id keys of the full range");
}

int main()
{
    named_cases();
    random_cases();
    rowptr_cases();
    limits();
    std::printf("%ld cases checked\n", cases_checked);
    std::printf("%d failures\n", failures);
    return failures != 0;
}
