// Host-side check of the filtered recommendation's plan (recommendersystems_amd/csrc/filter_plan.h), built against the header
// alone by tests/test_filter_plan.py: the bitmap and block geometry, the bitmap of a pool, the block offsets and the list of
// the candidate compaction against a direct walk over the rows, and every argument verdict in its order.  Prints every failure
// and exits non-zero if there is one.
#include "filter_plan.h"

#include <algorithm>
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

// ---- the bitmap, the block offsets, the list ------------------------------------------------------------------------------------

// pool == nullptr: no pool
static void check_list(const std::string &name, const std::vector<uint8_t> &types, int32_t t, const std::vector<int32_t> *pool)
{
    const int32_t n = (int32_t)types.size();
    const uint8_t *ty = types.empty() ? nullptr : types.data();
    // geometry: the words cover exactly the rows, every row has one bit of its own
    const size_t words = filter_bitmap_words(n);
    if (words * 32 < (size_t)n || (words > 0 && (words - 1) * 32 >= (size_t)n) || (n == 0 && words != 0)) fail(name + ": word count");
    std::set<std::pair<size_t, uint32_t>> seen;
    for (int32_t i = 0; i < n; ++i) {
        const uint32_t bit = filter_bit(i);
        if (filter_word(i) >= words || bit == 0 || (bit & (bit - 1)) != 0 || !seen.insert({filter_word(i), bit}).second) {
            fail(name + ": bit of row " + std::to_string(i));
            return;
        }
    }
    // the bitmap: exactly the listed rows
    std::vector<uint32_t> bm;
    std::set<int32_t> listed;
    if (pool) {
        bm = filter_bitmap(n, (int64_t)pool->size(), pool->empty() ? nullptr : pool->data());
        if (bm.size() != words) { fail(name + ": bitmap length"); return; }
        listed.insert(pool->begin(), pool->end());
        for (int32_t i = 0; i < n; ++i)
            if (((bm[filter_word(i)] & filter_bit(i)) != 0) != (listed.count(i) != 0)) { fail(name + ": bitmap at row " + std::to_string(i)); return; }
        // no bit beyond the last row
        if (words > 0 && (n & 31) != 0 && (bm[words - 1] >> (n & 31)) != 0) fail(name + ": a bit beyond the last row");
    }
    const uint32_t *b = pool ? bm.data() : nullptr;
    // brute force: the ascending list of the rows that match
    std::vector<int32_t> want;
    for (int32_t i = 0; i < n; ++i)
        if ((t == FILTER_ANY_TYPE || types[(size_t)i] == t) && (!pool || listed.count(i))) want.push_back(i);
    for (int32_t i = 0; i < n; ++i) {
        const bool m = std::binary_search(want.begin(), want.end(), i);
        if (filter_match(ty, t, b, i) != m) { fail(name + ": match of row " + std::to_string(i)); return; }
    }
    const int32_t nb = cand_blocks(n);
    const std::vector<int32_t> off = filter_block_offsets(ty, n, t, b);
    if (off.size() != (size_t)nb + 1) { fail(name + ": offset table length"); return; }
    for (int32_t k = 0; k <= nb; ++k) {
        const int32_t end = k < nb ? cand_block_lo(k) : n;
        const int32_t below = (int32_t)(std::lower_bound(want.begin(), want.end(), end) - want.begin());
        if (off[(size_t)k] != below) { fail(name + ": offset of block " + std::to_string(k)); return; }
    }
    const std::vector<int32_t> got = filter_list(ty, n, t, b, off);
    if (got != want) fail(name + ": the list is not the ascending, duplicate-free list of matches");
}

static void check_all_lists()
{
    std::mt19937_64 rng(7);
    for (int32_t n : {0, 1, 31, 32, 33, 255, 256, 257, 3 * 256 + 7}) {
        const std::string at = "n=" + std::to_string(n);
        std::vector<uint8_t> ones((size_t)n, 1), mixed((size_t)n);
        for (auto &x : mixed) x = (uint8_t)(rng() % 4);
        if (n > 0) mixed[(size_t)n - 1] = 2;
        std::vector<int32_t> all, none, edges, twice;
        for (int32_t i = 0; i < n; ++i) all.push_back(i);
        for (int32_t i : {0, 30, 31, 32, 33, 63, 64, 254, 255, 256, n - 2, n - 1})
            if (i >= 0 && i < n) edges.push_back(i);
        std::reverse(edges.begin(), edges.end());
        for (int32_t i : edges) { twice.push_back(i); twice.push_back(i); }
        std::shuffle(twice.begin(), twice.end(), rng);
        for (const std::vector<uint8_t> *ty : {&ones, &mixed})
            for (int32_t t : {FILTER_ANY_TYPE, 1, 2, 9}) {
                const std::string w = at + (ty == &ones ? " ones" : " mixed") + " type " + std::to_string(t);
                check_list(w + " no pool", *ty, t, nullptr);
                check_list(w + " empty pool", *ty, t, &none);
                check_list(w + " full pool", *ty, t, &all);
                check_list(w + " word edges, descending", *ty, t, &edges);
                check_list(w + " every member twice, shuffled", *ty, t, &twice);
                for (int it = 0; it < 4 && n > 0; ++it) {          // random pools with duplicates
                    std::vector<int32_t> p((size_t)(rng() % (2 * (uint64_t)n + 1)));
                    for (auto &x : p) x = (int32_t)(rng() % (uint64_t)n);
                    check_list(w + " random pool " + std::to_string(it), *ty, t, &p);
                }
            }
    }
    // more blocks than the scan takes per trip: the carry crosses chunks
    {
        const int32_t n = (CAND_SCAN_CHUNK + 3) * CAND_BLOCK + 5;
        std::vector<uint8_t> v((size_t)n);
        for (auto &x : v) x = (uint8_t)(rng() % 3);
        std::vector<int32_t> p((size_t)n / 3);
        for (auto &x : p) x = (int32_t)(rng() % (uint64_t)n);
        check_list("two scan chunks", v, 1, &p);
        check_list("two scan chunks, any type", v, FILTER_ANY_TYPE, &p);
    }
    // the marking launch: every entry of a pool is reached by its grid-stride walk, with at least one workgroup for one entry
    for (int64_t c : {(int64_t)-1, (int64_t)0, (int64_t)1, (int64_t)FILTER_MARK_BLOCK, (int64_t)FILTER_MARK_BLOCK + 1,
                      FILTER_MARK_BLOCKS_MAX * FILTER_MARK_BLOCK, FILTER_MARK_BLOCKS_MAX * FILTER_MARK_BLOCK + 1, (int64_t)1 << 40}) {
        const int32_t nb = filter_mark_blocks(c);
        const int64_t need = c > 0 ? (c + FILTER_MARK_BLOCK - 1) / FILTER_MARK_BLOCK : 0;
        if (nb != (need < FILTER_MARK_BLOCKS_MAX ? need : FILTER_MARK_BLOCKS_MAX) || (c > 0 && nb < 1))
            fail("marking workgroups for " + std::to_string(c) + " entries");
    }
}

// ---- the verdicts and their order --------------------------------------------------------------------------------------------

struct Args {
    bool graph = true;
    int32_t n = 10, K = 3, top_n = 5, top_max = 1024, cand = 2;
    uint32_t mask = 2;
    bool outs = true;
    std::vector<int32_t> seeds{0, 4, 9};
    bool null_seeds = false;
    int64_t pool_count = -1;
    std::vector<int32_t> pool;
    bool null_pool = true;
    std::vector<int64_t> deny_ptr;
    bool have_deny = false;
    std::vector<int32_t> deny_idx;
    bool null_deny_idx = false;
    std::vector<int64_t> test_ptr{0, 1, 1, 2};
    bool null_test_ptr = false;
    std::vector<int64_t> test_ids{7, 8};
    bool null_test_ids = false, pos_out = true;
};

static FilterCheck ranked(const Args &a)
{
    return filter_check(a.graph, a.n, a.null_seeds ? nullptr : a.seeds.data(), a.K, a.top_n, a.top_max, a.cand, a.mask, a.outs,
                        a.pool_count, a.null_pool ? nullptr : a.pool.data(), a.have_deny ? a.deny_ptr.data() : nullptr,
                        a.null_deny_idx ? nullptr : a.deny_idx.data());
}

static FilterCheck positions(const Args &a)
{
    static int dummy;
    return filter_positions_check(a.graph, a.n, a.null_seeds ? nullptr : a.seeds.data(), a.K, a.cand, a.mask, a.pool_count,
                                  a.null_pool ? nullptr : a.pool.data(), a.have_deny ? a.deny_ptr.data() : nullptr,
                                  a.null_deny_idx ? nullptr : a.deny_idx.data(), a.null_test_ptr ? nullptr : a.test_ptr.data(),
                                  a.null_test_ids ? nullptr : a.test_ids.data(), a.pos_out ? &dummy : nullptr);
}

// One fault per step of the documented order, each applied on top of all LATER ones: the earliest must win.
static void check_verdicts()
{
    struct Step {
        const char *name;
        void (*breakit)(Args &);
        FilterVerdict v;
        int32_t typed, deny, test;       // the part verdict expected with it
        bool ranked_only, positions_only;
    };
    const std::vector<Step> steps = {
        {"NULL graph", [](Args &a) { a.graph = false; }, FILTER_TYPED, TYPED_NULL_GRAPH, 0, 0, false, false},
        {"negative K", [](Args &a) { a.K = -1; }, FILTER_TYPED, TYPED_NEGATIVE_K, 0, 0, false, false},
        {"NULL seeds", [](Args &a) { a.null_seeds = true; }, FILTER_TYPED, TYPED_NULL_ARG, 0, 0, false, false},
        {"NULL outputs", [](Args &a) { a.outs = false; }, FILTER_TYPED, TYPED_NULL_ARG, 0, 0, true, false},
        {"top_n 0", [](Args &a) { a.top_n = 0; }, FILTER_TYPED, TYPED_BAD_TOP_N, 0, 0, true, false},
        {"cand_type -2", [](Args &a) { a.cand = -2; }, FILTER_TYPED, TYPED_BAD_CAND_TYPE, 0, 0, false, false},
        {"mask bit 8", [](Args &a) { a.mask = 1u << 8; }, FILTER_TYPED, TYPED_BAD_MASK, 0, 0, false, false},
        {"seed out of range", [](Args &a) { a.seeds[1] = a.n; }, FILTER_TYPED, TYPED_SEED_RANGE, 0, 0, false, false},
        {"NULL pool", [](Args &a) { a.pool_count = 2; a.null_pool = true; }, FILTER_NULL_POOL, 0, 0, 0, false, false},
        {"pool index out of range", [](Args &a) { a.pool_count = 3; a.pool = {1, 1, a.n}; a.null_pool = false; }, FILTER_POOL_RANGE, 0, 0, 0,
         false, false},
        {"deny_ptr[0]", [](Args &a) { a.have_deny = true; a.deny_ptr = {1, 1, 1, 1}; a.deny_idx = {0}; }, FILTER_DENY, 0, EXCLUDE_BAD_PTR0, 0,
         false, false},
        {"deny_ptr decreases", [](Args &a) { a.have_deny = true; a.deny_ptr = {0, 2, 1, 2}; a.deny_idx = {0, 1}; }, FILTER_DENY, 0,
         EXCLUDE_PTR_DECREASES, 0, false, false},
        {"NULL deny_idx", [](Args &a) { a.have_deny = true; a.deny_ptr = {0, 1, 1, 2}; a.null_deny_idx = true; }, FILTER_DENY, 0,
         EXCLUDE_NULL_IDX, 0, false, false},
        {"deny index out of range", [](Args &a) { a.have_deny = true; a.deny_ptr = {0, 1, 1, 2}; a.deny_idx = {3, -1}; a.null_deny_idx = false; },
         FILTER_DENY, 0, EXCLUDE_BAD_INDEX, 0, false, false},
        {"NULL test_ptr", [](Args &a) { a.null_test_ptr = true; }, FILTER_TEST, 0, 0, EVAL_NULL_PTR, false, true},
        {"NULL pos_out", [](Args &a) { a.pos_out = false; }, FILTER_TEST, 0, 0, EVAL_NULL_OUT, false, true},
        {"test_ptr[0]", [](Args &a) { a.test_ptr = {1, 1, 1, 2}; }, FILTER_TEST, 0, 0, EVAL_BAD_PTR0, false, true},
        {"test_ptr decreases", [](Args &a) { a.test_ptr = {0, 2, 1, 2}; }, FILTER_TEST, 0, 0, EVAL_PTR_DECREASES, false, true},
        {"NULL test_ids", [](Args &a) { a.null_test_ids = true; }, FILTER_TEST, 0, 0, EVAL_NULL_IDS, false, true},
        {"top_n beyond the limit", [](Args &a) { a.top_n = a.top_max + 1; }, FILTER_TOP_N_LIMIT, 0, 0, 0, true, false},
    };
    for (int pos = 0; pos < 2; ++pos)
        for (size_t first = 0; first < steps.size(); ++first) {
            const Step &s = steps[first];
            if (pos ? s.ranked_only : s.positions_only) continue;
            // the later faults first, the one under test last, so that no later step's edit repairs it
            Args a;
            for (size_t later = steps.size(); later-- > first + 1;) {
                const Step &l = steps[later];
                if (pos ? l.ranked_only : l.positions_only) continue;
                if (l.v == s.v && l.v != FILTER_TYPED) continue;   // (one set description holds one fault at a time)
                l.breakit(a);
            }
            s.breakit(a);
            const FilterCheck c = pos ? positions(a) : ranked(a);
            const std::string w = std::string(pos ? "positions: " : "ranked: ") + s.name;
            if (c.verdict != s.v) { fail(w + ": verdict " + std::to_string((int)c.verdict)); continue; }
            if (s.v == FILTER_TYPED && (int32_t)c.typed.verdict != s.typed) fail(w + ": typed verdict " + std::to_string((int)c.typed.verdict));
            if (s.v == FILTER_DENY && (int32_t)c.deny.verdict != s.deny) fail(w + ": deny verdict " + std::to_string((int)c.deny.verdict));
            if (s.v == FILTER_TEST && (int32_t)c.test.verdict != s.test) fail(w + ": test verdict " + std::to_string((int)c.test.verdict));
        }
    // the positions reported with the range verdicts
    {
        Args a;
        a.seeds = {0, -1, 99};
        FilterCheck c = ranked(a);
        if (c.verdict != FILTER_TYPED || c.typed.bad_k != 1 || c.typed.bad_seed != -1) fail("seed range: first offender");
        a = Args();
        a.pool_count = 5, a.pool = {3, 3, -7, 10, 2}, a.null_pool = false;
        c = ranked(a);
        if (c.verdict != FILTER_POOL_RANGE || c.bad_pos != 2 || c.bad_index != -7) fail("pool range: first offender");
        a.pool = {3, 3, 9, 10, 2};
        c = positions(a);
        if (c.verdict != FILTER_POOL_RANGE || c.bad_pos != 3 || c.bad_index != 10) fail("pool range: n itself");
        a = Args();
        a.have_deny = true, a.deny_ptr = {0, 2, 2, 4}, a.deny_idx = {0, 9, 9, 10};
        c = ranked(a);
        if (c.verdict != FILTER_DENY || c.deny.verdict != EXCLUDE_BAD_INDEX || c.deny.bad_k != 2 || c.deny.bad_index != 10)
            fail("deny range: batch position");
    }
    // what passes: K == 0 (whatever else is wrong behind it, a graph given), cand_type -1 and 255, every legal pool shape, deny
    // lists with duplicates, the seed, empty lists; top_n at the limit
    {
        Args a;
        a.K = 0, a.null_seeds = true, a.outs = false, a.top_n = 0, a.cand = -9, a.pool_count = 4, a.null_pool = true;
        if (ranked(a).verdict != FILTER_NOOP || positions(a).verdict != FILTER_NOOP) fail("K == 0 is a no-op");
        a.graph = false;
        if (ranked(a).verdict != FILTER_TYPED || ranked(a).typed.verdict != TYPED_NULL_GRAPH) fail("a NULL graph before the no-op");
        for (int32_t cand : {-1, 0, 255}) {
            a = Args();
            a.cand = cand;
            if (ranked(a).verdict != FILTER_OK || positions(a).verdict != FILTER_OK) fail("cand_type " + std::to_string(cand) + " passes");
        }
        a = Args();
        a.cand = 256;
        if (ranked(a).verdict != FILTER_TYPED || ranked(a).typed.verdict != TYPED_BAD_CAND_TYPE) fail("cand_type 256");
        a = Args();
        a.pool_count = 0, a.null_pool = true;                      // an empty pool needs no array
        if (ranked(a).verdict != FILTER_OK || positions(a).verdict != FILTER_OK) fail("an empty pool passes");
        a.pool_count = -5;                                         // no pool: the array is not read
        if (ranked(a).verdict != FILTER_OK) fail("no pool passes");
        a.pool_count = 6, a.pool = {9, 0, 9, 0, 4, 4}, a.null_pool = false;
        a.have_deny = true, a.deny_ptr = {0, 3, 3, 5}, a.deny_idx = {0, 0, 7, 9, 9};
        a.top_n = a.top_max;
        if (ranked(a).verdict != FILTER_OK || positions(a).verdict != FILTER_OK) fail("a legal pool and deny lists pass");
        a.deny_ptr = {0, 0, 0, 0}, a.null_deny_idx = true;          // empty deny lists need no index array
        if (ranked(a).verdict != FILTER_OK) fail("empty deny lists pass");
        a.top_n = a.top_max + 1;
        if (ranked(a).verdict != FILTER_TOP_N_LIMIT) fail("top_n limit alone");
        if (positions(a).verdict != FILTER_OK) fail("the positions entry has no top_n");
    }
}

int main()
{
    check_all_lists();
    check_verdicts();
    std::printf("%d failures\n", failures);
    return failures != 0;
}
