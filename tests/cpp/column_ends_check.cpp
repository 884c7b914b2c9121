// Host-side check of the column ends of a tile group of Models (recommendersystems_amd/csrc/column_ends.h), built against
// the header alone by tests/test_column_ends.py.  ColumnEnds is driven the way the batch drivers drive it -- due(), leaving(),
// done() before each step, stuck() once the step limit is reached -- over scripted distances, and compared with a direct
// per-column simulation: column k ends after the first step s >= 1 with dist_s[k] < threshold, or after step T in iteration
// mode.  Prints every failure and exits non-zero if there is one.
#include "column_ends.h"

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

// K columns dealt to ntiles tiles of G slots as the drivers deal them (position r in slot (r % ntiles) * G + r / ntiles, the
// rest padding)
static std::vector<int32_t> deal(int32_t K, int G)
{
    const size_t ntiles = ((size_t)K + G - 1) / G;
    std::vector<int32_t> slot_k(ntiles * G, -1);
    for (int32_t k = 0; k < K; ++k) slot_k[(size_t)(k % ntiles) * G + (size_t)(k / ntiles)] = k;
    return slot_k;
}

constexpr int64_t UNSET = -7;

// dist[s - 1][q] = slot q's distance after step s (threshold modes; T rows).  with_iters = false: iters_out is NULL.
// Returns the step after which the group stopped.
static int64_t check_case(const std::string &name, const std::vector<int32_t> &slot_k, bool by_count, int64_t T, double threshold,
                          const std::vector<std::vector<double>> &dist, bool with_iters = true)
{
    const size_t nslots = slot_k.size();
    int32_t K = 0, real = 0;
    for (int32_t k : slot_k) { K = k + 1 > K ? k + 1 : K; real += k >= 0; }
    // the simulation: the step after which each slot's column ends, -1 = never within T steps
    std::vector<int64_t> want(nslots, -1);
    int32_t want_stuck = -1;
    for (size_t q = 0; q < nslots; ++q) {
        if (slot_k[q] < 0) continue;
        if (by_count) want[q] = T;
        for (int64_t s = 1; !by_count && s <= T && want[q] < 0; ++s)
            if (dist[(size_t)s - 1][q] < threshold) want[q] = s;
        if (want[q] < 0 && (want_stuck < 0 || slot_k[q] < want_stuck)) want_stuck = slot_k[q];
    }

    ColumnEnds ce(slot_k.data(), nslots, by_count, T, threshold);
    if (ce.real != real || ce.live != real) fail(name + ": real / live after construction");
    std::vector<int64_t> iters((size_t)K, UNSET);
    std::vector<int32_t> row_of(nslots, 99), emitted(nslots, 0);
    int32_t left = 0;
    int64_t steps = 0;
    for (;;) {
        int32_t want_m = 0;
        for (size_t q = 0; q < nslots; ++q) want_m += slot_k[q] >= 0 && want[q] == steps;
        if (ce.due(steps)) {
            const double *d = by_count ? nullptr : dist[(size_t)steps - 1].data();   // (iteration mode reads no distance)
            const int32_t m = ce.leaving(steps, d, row_of.data(), with_iters ? iters.data() : nullptr);
            if (m != want_m) fail(name + ": step " + std::to_string(steps) + ": " + std::to_string(m) + " columns leave, " + std::to_string(want_m) + " expected");
            int32_t next = 0;
            for (size_t q = 0; q < nslots; ++q) {
                const bool leaves = slot_k[q] >= 0 && want[q] == steps;
                if (row_of[q] != (leaves ? next : -1)) fail(name + ": step " + std::to_string(steps) + ": row_of[" + std::to_string(q) + "] = " + std::to_string(row_of[q]));
                if (leaves) { ++next; ++emitted[q]; }
            }
            left += m;
            if (ce.live != real - left) fail(name + ": live after step " + std::to_string(steps));
            if (ce.done() != (left == real)) fail(name + ": done() after step " + std::to_string(steps));
            if (ce.done()) break;
        } else if (want_m != 0) {
            fail(name + ": due() is false at step " + std::to_string(steps) + ", where a column ends");
        }
        if (steps == T) break;
        ++steps;
    }
    if (ce.stuck() != want_stuck) fail(name + ": stuck() = " + std::to_string(ce.stuck()) + ", " + std::to_string(want_stuck) + " expected");
    if ((want_stuck < 0) != ce.done()) fail(name + ": done() at the end");
    for (size_t q = 0; q < nslots; ++q) {
        if (emitted[q] != (slot_k[q] >= 0 && want[q] >= 0 && want[q] <= steps)) fail(name + ": slot " + std::to_string(q) + " emitted " + std::to_string(emitted[q]) + " times");
        if (slot_k[q] < 0) continue;
        const int64_t w = with_iters && want[q] >= 0 ? want[q] : UNSET;
        if (iters[(size_t)slot_k[q]] != w) fail(name + ": iters[" + std::to_string(slot_k[q]) + "] = " + std::to_string(iters[(size_t)slot_k[q]]));
    }
    return steps;
}

// distances that fall below 1e-9 from step stop[q] on (stop 0: never)
static std::vector<std::vector<double>> falling(const std::vector<int64_t> &stop, int64_t T)
{
    std::vector<std::vector<double>> d((size_t)T, std::vector<double>(stop.size(), 1.0));
    for (int64_t s = 1; s <= T; ++s)
        for (size_t q = 0; q < stop.size(); ++q)
            if (stop[q] > 0 && s >= stop[q]) d[(size_t)s - 1][q] = 1e-12;
    return d;
}

int main()
{
    // iteration mode, T = 0: every real column leaves at step 0 with iters 0; due() is false at every other step
    {
        const std::vector<int32_t> slot_k = {0, 1, 2, -1};
        if (check_case("T = 0", slot_k, true, 0, 0.0, {}) != 0) fail("T = 0: not stopped at step 0");
        ColumnEnds ce(slot_k.data(), slot_k.size(), true, 0, 0.0);
        if (!ce.due(0)) fail("T = 0: due(0)");
        for (int64_t s = 1; s < 6; ++s)
            if (ce.due(s)) fail("T = 0: due(" + std::to_string(s) + ")");
    }
    // iteration mode, T = 3, K = 5 in 2 tiles of 4: row_of numbers the real slots only, in slot order
    {
        const std::vector<int32_t> slot_k = deal(5, 4);
        const std::vector<int32_t> dealt = {0, 2, 4, -1, 1, 3, -1, -1}, rows = {0, 1, 2, -1, 3, 4, -1, -1};
        if (slot_k != dealt) fail("T = 3: the dealing");
        if (check_case("T = 3", slot_k, true, 3, 0.0, {}) != 3) fail("T = 3: not stopped at step 3");
        check_case("T = 3, NULL iters_out", slot_k, true, 3, 0.0, {}, false);
        ColumnEnds ce(slot_k.data(), slot_k.size(), true, 3, 0.0);
        std::vector<int32_t> row_of(8, 99);
        std::vector<int64_t> iters(5, UNSET);
        for (int64_t s = 0; s < 3; ++s)
            if (ce.due(s)) fail("T = 3: due(" + std::to_string(s) + ")");
        if (ce.leaving(3, nullptr, row_of.data(), iters.data()) != 5 || row_of != rows) fail("T = 3: row_of");
        if (iters != std::vector<int64_t>(5, 3) || !ce.done() || ce.stuck() != -1) fail("T = 3: iters / done / stuck");
        // ... and as two tile groups of one tile
        check_case("T = 3, first tile", {0, 2, 4, -1}, true, 3, 0.0, {});
        check_case("T = 3, second tile", {1, 3, -1, -1}, true, 3, 0.0, {});
    }
    // threshold mode: stops at steps 1, 3, 3, 5 and 2; the column of slot 6 dips below the threshold at step 2, rises above it
    // at steps 3 and 4 and falls again at 6 -- it leaves once, after step 2.  Slot 2 is padding.
    {
        const std::vector<int32_t> slot_k = {4, 0, -1, 5, 2, 1, 3, -1};
        const std::vector<int64_t> stop = {1, 3, 1, 3, 5, 2, 2, 0};
        auto d = falling(stop, 8);
        d[2][6] = d[3][6] = 0.5;
        if (check_case("distinct stops", slot_k, false, 8, 1e-9, d) != 5) fail("distinct stops: not stopped after step 5");
        check_case("distinct stops, NULL iters_out", slot_k, false, 8, 1e-9, d, false);
        // the step limit before the last stop: batch position 2 (slot 4) is stuck
        if (check_case("distinct stops, T = 4", slot_k, false, 4, 1e-9, d) != 4) fail("distinct stops, T = 4: steps");
        // a distance equal to the threshold does not end a column (Model.cs:64 is <)
        auto e = falling({2}, 3);
        e[1][0] = 1e-9;
        if (check_case("equal to the threshold", {0}, false, 3, 1e-9, e) != 3) fail("equal to the threshold");
    }
    // threshold 0.0: nothing ever leaves (not even a distance of 0.0); stuck() is the smallest batch position, which is
    // not in the first slot here
    {
        const std::vector<int32_t> slot_k = {3, 1, -1, 2};
        auto d = falling({0, 0, 0, 0}, 4);
        d[1][1] = 0.0;
        if (check_case("threshold 0", slot_k, false, 4, 0.0, d) != 4) fail("threshold 0: steps");
        ColumnEnds ce(slot_k.data(), slot_k.size(), false, 4, 0.0);
        std::vector<int32_t> row_of(4);
        for (int64_t s = 1; s <= 4; ++s)
            if (!ce.due(s) || ce.leaving(s, d[(size_t)s - 1].data(), row_of.data(), nullptr) != 0) fail("threshold 0: a column left");
        if (ce.stuck() != 1 || ce.done()) fail("threshold 0: stuck() = " + std::to_string(ce.stuck()));
    }
    // A group of padding slots alone.  Neither driver makes one: both deal position r < ntiles to the first slot of tile r,
    // and ntiles <= K -- the precondition column_ends.h documents, checked here for every dealing.  ColumnEnds itself
    // then has nothing to wait for: done() before any step.
    for (int32_t K = 1; K <= 40; ++K)
        for (int G : {1, 2, 4, 8, 16}) {
            const std::vector<int32_t> slot_k = deal(K, G);
            for (size_t t = 0; t < slot_k.size(); t += (size_t)G) {
                const ColumnEnds ce(slot_k.data() + t, (size_t)G, true, 1, 0.0);
                if (slot_k[t] < 0 || ce.real == 0 || ce.done()) fail("dealing K = " + std::to_string(K) + " G = " + std::to_string(G) + ": a tile without a column");
            }
        }
    {
        const std::vector<int32_t> slot_k(4, -1);
        const ColumnEnds ce(slot_k.data(), slot_k.size(), false, 5, 1e-9);
        if (!ce.done() || ce.real != 0 || ce.stuck() != -1) fail("padding only");
    }

    std::mt19937_64 rng(11);
    for (int it = 0; it < 400; ++it) {
        const int G = 1 << (rng() % 4);
        const int32_t K = 1 + (int32_t)(rng() % 20);
        const std::vector<int32_t> all = deal(K, G);
        const size_t tiles = all.size() / G, tg = 1 + (size_t)(rng() % tiles), t0 = (size_t)(rng() % (tiles - tg + 1));
        const std::vector<int32_t> slot_k(all.begin() + (long)(t0 * G), all.begin() + (long)((t0 + tg) * G));
        const bool by_count = rng() % 3 == 0;
        const int64_t T = (int64_t)(rng() % 7);
        std::vector<std::vector<double>> d((size_t)T, std::vector<double>(slot_k.size()));
        for (auto &row : d)
            for (auto &x : row) x = (rng() % 4 == 0) ? 1e-12 : 1.0;             // (rises again at random)
        check_case("random " + std::to_string(it), slot_k, by_count, T, rng() % 8 == 0 ? 0.0 : 1e-9, d, rng() % 2 == 0);
    }
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
