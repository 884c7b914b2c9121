// Host-side check of the filtered recommendation's plan (recommendersystems_amd/csrc/filter_plan.h), built against the header
// alone by tests/test_filter_plan.py: the bitmap and block geometry, the bitmap of a pool, and the block offsets and the list of
// the candidate compaction against a direct walk over the rows.  (The argument verdicts: tests/cpp/typed_call_check.cpp.)
// Prints every failure and exits non-zero if there is one.
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

int main()
{
    check_all_lists();
    std::printf("%d failures\n", failures);
    return failures != 0;
}
