// Host-side check of the removal plan (recommendersystems_amd/csrc/remove_plan.h) and of the index arithmetic of the device
// compaction (the rm_* functions there and the segment copies of seg_copy.h, the very code k_remove_compact compiles), built
// against the headers alone by tests/test_remove_plan.py.  Every case is compared with a brute-force list-of-lists erase
// (edges[src].RemoveAt(k)); the compaction is replayed workgroup by workgroup and lane by lane, once in launch order and once
// in the reverse order, and counted: every new position written exactly once, no removed position read.
// Prints every failure and exits non-zero if there is one.
#include "remove_plan.h"
#include "seg_copy.h"

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

// an element that counts how often it is read and written: copy_seg<Traced> is the code that copies weights and targets
struct Traced {
    int64_t val = -1;
    mutable int reads = 0;
    int writes = 0;
    Traced() = default;
    Traced(const Traced &o) : val(o.val) { ++o.reads; }
    Traced &operator=(const Traced &o)
    {
        val = o.val;
        ++o.reads;
        ++writes;
        return *this;
    }
};

static uint8_t byte_of(int64_t e) { return (uint8_t)((e * 7 + 3) % 251); }   // (never 0xFF: the mark of a removed position)

struct Replay {
    std::vector<Traced> w_o, w_n;
    std::vector<uint8_t> et_o, et_n;
    int64_t sparse_chunks = 0, dense_chunks = 0;
    std::vector<int> path;             // per chunk: 0 sparse, 1 dense
};

// k_remove_compact on the host: the workgroups and the lanes of a workgroup one after the other, forwards or backwards
static Replay replay(int64_t m_old, const std::vector<int64_t> &r, bool backwards)
{
    const int64_t nr = (int64_t)r.size(), m_new = m_old - nr;
    Replay R;
    R.w_o.resize((size_t)m_old);
    R.et_o.resize((size_t)m_old);
    for (int64_t e = 0; e < m_old; ++e) { R.w_o[(size_t)e].val = e; R.et_o[(size_t)e] = byte_of(e); }
    for (int64_t k = 0; k < nr; ++k) R.et_o[(size_t)r[(size_t)k]] = 0xFF;
    R.w_n.resize((size_t)(m_new > 0 ? m_new : 1));
    R.et_n.assign((size_t)(m_new > 0 ? m_new : 1), 0xEE);
    const int64_t chunks = (m_old + RM_CHUNK - 1) / RM_CHUNK;
    R.path.assign((size_t)chunks, 0);
    for (int64_t cc = 0; cc < chunks; ++cc) {
        const int64_t c = backwards ? chunks - 1 - cc : cc;
        const int64_t c0 = c * RM_CHUNK, c1 = std::min<int64_t>(c0 + RM_CHUNK, m_old);
        const RmSlice s = rm_chunk_slice(r.data(), nr, c0, c1);
        if (rm_chunk_dense(s)) {
            ++R.dense_chunks;
            R.path[(size_t)c] = 1;
            for (int tt = 0; tt < SEG_THREADS; ++tt) {
                const int tid = backwards ? SEG_THREADS - 1 - tt : tt;
                for (int64_t e = c0 + tid; e < c1; e += SEG_THREADS) {
                    int64_t to;
                    if (!rm_dense_dest(r.data(), s, e, &to)) continue;
                    if (to < 0 || to >= m_new) { fail("dense destination outside [0, m_new)"); continue; }
                    R.w_n[(size_t)to] = R.w_o[(size_t)e];
                    R.et_n[(size_t)to] = R.et_o[(size_t)e];
                }
            }
            continue;
        }
        ++R.sparse_chunks;
        const int64_t segs = s.jend - s.j + 1;
        for (int64_t tq = 0; tq < segs; ++tq) {
            const int64_t t = backwards ? segs - 1 - tq : tq;
            const RmSeg g = rm_segment(r.data(), s, c0, c1, t);
            if (g.b < g.a) fail("segment ends before it starts");
            if (g.b <= g.a) continue;
            if (g.a < c0 || g.b > c1 || g.a - g.sh < 0 || g.b - g.sh > m_new) { fail("segment outside its chunk or its image outside [0, m_new)"); continue; }
            for (int tt = 0; tt < SEG_THREADS; ++tt) {
                const int tid = backwards ? SEG_THREADS - 1 - tt : tt;
                copy_seg<Traced>(R.w_o.data(), R.w_n.data(), g.a, g.b, -g.sh, tid);
                copy_seg_bytes(R.et_o.data(), R.et_n.data(), g.a, g.b, -g.sh, tid);
            }
        }
    }
    return R;
}

// deg[i] links per row, the links at the flat positions idx removed: checks every output of the plan and the replay of the
// compaction against the lists.  Returns the forward replay (for the cases that look at the path taken).
static Replay check_case(const std::string &name, const std::vector<int64_t> &deg, const std::vector<int64_t> &idx)
{
    const int32_t n = (int32_t)deg.size();
    const int64_t count = (int64_t)idx.size();
    std::vector<int64_t> rowptr((size_t)n + 1, 0);
    for (int32_t i = 0; i < n; ++i) rowptr[(size_t)i + 1] = rowptr[i] + deg[i];
    const int64_t m = rowptr[n];

    // brute force: the lists of old flat positions, erased from (largest position first, so that the others stay put)
    std::vector<std::vector<int64_t>> lists((size_t)n);
    for (int32_t i = 0; i < n; ++i)
        for (int64_t e = rowptr[i]; e < rowptr[(size_t)i + 1]; ++e) lists[i].push_back(e);
    std::vector<int64_t> desc(idx);
    std::sort(desc.begin(), desc.end(), [](int64_t a, int64_t b) { return a > b; });
    for (int64_t e : desc) {
        const int32_t i = (int32_t)(std::upper_bound(rowptr.begin(), rowptr.end(), e) - rowptr.begin()) - 1;
        lists[(size_t)i].erase(lists[(size_t)i].begin() + (e - rowptr[(size_t)i]));
    }
    std::vector<int64_t> flat, rowptr_new((size_t)n + 1, 0);
    for (int32_t i = 0; i < n; ++i) {
        for (int64_t e : lists[i]) flat.push_back(e);
        rowptr_new[(size_t)i + 1] = (int64_t)flat.size();
    }

    const RemovePlan p = remove_plan(n, rowptr.data(), count, idx.data());
    if (p.verdict != REMOVE_OK) { fail(name + ": verdict " + std::to_string((int)p.verdict)); return Replay{}; }
    if (p.m_old != m || p.m_new != m - count) fail(name + ": m_old / m_new");
    std::vector<int64_t> asc(idx);
    std::sort(asc.begin(), asc.end());
    if (p.r != asc) { fail(name + ": r is not the removed positions ascending"); return Replay{}; }
    if (p.rowptr_new != rowptr_new) fail(name + ": rowptr_new");
    for (int32_t i = 0; i <= n; ++i)
        if (rm_rowptr_new(p.r.data(), count, rowptr[(size_t)i]) != rowptr_new[(size_t)i]) { fail(name + ": rm_rowptr_new at " + std::to_string(i)); break; }
    for (size_t q = 0; q < flat.size(); ++q)
        if (flat[q] - p.shift(flat[q]) != (int64_t)q) { fail(name + ": shift of old position " + std::to_string(flat[q])); break; }

    Replay fwd;
    for (int pass = 0; pass < 2; ++pass) {
        Replay R = replay(m, p.r, pass == 1);
        const std::string where = name + (pass ? " (backwards)" : " (forwards)");
        bool ok = true;
        for (size_t q = 0; q < flat.size() && ok; ++q) {
            if (R.w_n[q].writes != 1) { fail(where + ": new position " + std::to_string(q) + " written " + std::to_string(R.w_n[q].writes) + " times"); ok = false; }
            else if (R.w_n[q].val != flat[q]) { fail(where + ": new position " + std::to_string(q) + " holds the wrong link"); ok = false; }
            else if (R.et_n[q] != byte_of(flat[q])) { fail(where + ": type byte at new position " + std::to_string(q)); ok = false; }
        }
        for (int64_t e = 0; e < m && ok; ++e) {
            const bool removed = std::binary_search(asc.begin(), asc.end(), e);
            if (R.w_o[(size_t)e].reads != (removed ? 0 : 1)) { fail(where + ": old position " + std::to_string(e) + " read " + std::to_string(R.w_o[(size_t)e].reads) + " times"); ok = false; }
        }
        if (pass == 0) fwd = std::move(R);
    }
    return fwd;
}

static std::vector<int64_t> iota_vec(int64_t a, int64_t b)   // a, a + 1, ..., b - 1
{
    std::vector<int64_t> v;
    for (int64_t e = a; e < b; ++e) v.push_back(e);
    return v;
}

static void check_verdict(const std::string &name, const std::vector<int64_t> &deg, const std::vector<int64_t> &idx, int64_t count,
                          RemoveVerdict want, int64_t want_q)
{
    const int32_t n = (int32_t)deg.size();
    std::vector<int64_t> rowptr((size_t)n + 1, 0);
    for (int32_t i = 0; i < n; ++i) rowptr[(size_t)i + 1] = rowptr[i] + deg[i];
    const RemovePlan p = remove_plan(n, rowptr.data(), count, idx.empty() ? nullptr : idx.data());
    if (p.verdict != want || p.bad_q != want_q)
        fail(name + ": verdict " + std::to_string((int)p.verdict) + " at q = " + std::to_string(p.bad_q) + ", expected " +
             std::to_string((int)want) + " at " + std::to_string(want_q));
    if (p.verdict != REMOVE_OK && (p.m_new != p.m_old || !p.r.empty() || !p.rowptr_new.empty())) fail(name + ": a refused plan carries tables");
}

static void check_sort(const std::string &name, int64_t m_old, int64_t count, int passes, std::mt19937_64 &rng)
{
    int expect = 0;
    for (int sh = 0; ((m_old - 1) >> sh) > 0; sh += 11) ++expect;
    if (expect != passes) fail(name + ": the case does not take " + std::to_string(passes) + " passes");
    std::vector<int64_t> idx((size_t)count);
    for (int64_t &v : idx) v = (int64_t)(rng() % (uint64_t)m_old);
    idx[0] = m_old - 1;
    idx[1] = 0;
    idx[2] = idx[3];                                          // (equal keys: stability shows)
    std::vector<int64_t> order, want((size_t)count);
    remove_order_by_position(m_old, count, idx.data(), order);
    for (int64_t q = 0; q < count; ++q) want[(size_t)q] = q;
    std::stable_sort(want.begin(), want.end(), [&](int64_t a, int64_t b) { return idx[(size_t)a] < idx[(size_t)b]; });
    if (order != want) fail(name + ": order differs from std::stable_sort");
}

int main()
{
    std::mt19937_64 rng(20260101);
    // ---- small lists
    check_case("count 0", {3, 0, 2}, {});
    check_case("count 0, no links at all", {0, 0, 0}, {});
    check_case("one position", {3, 0, 2}, {1});
    check_case("one link, removed", {0, 1, 0}, {0});
    check_case("positions 0 and m-1", {3, 0, 2, 4}, {0, 8});
    {
        const std::vector<int64_t> deg = {0, 0, 4, 0, 3, 0, 0, 5, 2, 0, 0};   // rows already empty before, between and behind
        check_case("whole first non-empty row", deg, iota_vec(0, 4));
        check_case("whole middle row", deg, iota_vec(4, 7));
        check_case("whole last non-empty row", deg, iota_vec(12, 14));
        check_case("whole rows 2 and 7", deg, {7, 0, 8, 1, 9, 2, 10, 3, 11});
        check_case("every link", deg, iota_vec(0, 14));
        check_case("row 0 whole", {4, 0, 3}, iota_vec(0, 4));
        check_case("row n-1 whole", {4, 0, 3}, iota_vec(4, 7));
        check_case("descending", deg, {13, 9, 8, 4, 0});
        check_case("shuffled", deg, {5, 12, 0, 9, 3, 10, 7});
    }
    // ---- lists of several chunks: 2 * 8 192 + 100 links (a last chunk shorter than 8 192), rows of 1 000 with empty ones
    std::vector<int64_t> big;
    for (int i = 0; i < 16; ++i) { big.push_back(1000); if (i % 3 == 0) big.push_back(0); }
    big.push_back(484);
    const int64_t M = 2 * RM_CHUNK + 100;
    {
        int64_t sum = 0;
        for (int64_t d : big) sum += d;
        if (sum != M) fail("the chunked cases' link count");
    }
    {
        const Replay R = check_case("count 0, three chunks", big, {});
        if (R.sparse_chunks != 3 || R.dense_chunks != 0) fail("count 0: three sparse chunks expected");
    }
    check_case("run across a chunk boundary", big, {8190, 8191, 8192, 8193, 8194});
    check_case("first and last of every chunk", big, {0, 8191, 8192, 16383, 16384, M - 1});
    check_case("last chunk: its end", big, {M - 1, M - 2, M - 100});
    check_case("last chunk removed whole", big, iota_vec(2 * RM_CHUNK, M));
    {
        const Replay R = check_case("a chunk removed whole", big, iota_vec(RM_CHUNK, 2 * RM_CHUNK));
        if (R.path[1] != 1) fail("a chunk removed whole takes the dense path");
    }
    check_case("every link, three chunks", big, iota_vec(0, M));
    {
        // exactly 32 removed positions in chunk 0 (sparse), exactly 33 in chunk 1 (dense), one in chunk 2
        std::vector<int64_t> idx;
        for (int k = 0; k < 32; ++k) idx.push_back(5 + 251 * k);
        for (int k = 0; k < 33; ++k) idx.push_back(RM_CHUNK + 17 + 240 * k);
        idx.push_back(2 * RM_CHUNK + 50);
        std::shuffle(idx.begin(), idx.end(), rng);
        const Replay R = check_case("32 and 33 in a chunk", big, idx);
        if (R.path != std::vector<int>{0, 1, 0}) fail("32 removed positions are sparse, 33 dense");
    }
    {
        // 32 consecutive ones (empty segments in between) stay sparse
        const Replay R = check_case("32 neighbours", big, iota_vec(100, 132));
        if (R.path[0] != 0) fail("32 neighbouring positions take the sparse path");
    }
    // ---- random cases: small lists, then chunked ones of every density
    for (int c = 0; c < 300; ++c) {
        const int n = 1 + (int)(rng() % 12);
        std::vector<int64_t> deg((size_t)n);
        int64_t m = 0;
        for (int64_t &d : deg) { d = (int64_t)(rng() % 6); m += d; }
        std::vector<int64_t> all = iota_vec(0, m);
        std::shuffle(all.begin(), all.end(), rng);
        all.resize((size_t)(m > 0 ? rng() % (uint64_t)(m + 1) : 0));
        check_case("random small " + std::to_string(c), deg, all);
    }
    for (int c = 0; c < 24; ++c) {
        const int n = 5 + (int)(rng() % 60);
        std::vector<int64_t> deg((size_t)n);
        int64_t m = 0;
        for (int64_t &d : deg) { d = (rng() % 4 == 0) ? 0 : (int64_t)(rng() % 900); m += d; }
        if (m == 0) continue;
        std::vector<int64_t> all = iota_vec(0, m);
        std::shuffle(all.begin(), all.end(), rng);
        const int64_t counts[6] = {1, 7, 40, 200, m / 3, m - 1};
        all.resize((size_t)std::min<int64_t>(counts[c % 6], m));
        check_case("random chunked " + std::to_string(c), deg, all);
    }
    // ---- the radix sort at link counts taking one, two and three passes; a plan at the largest
    check_sort("sort, one pass", 2000, 3000, 1, rng);
    check_sort("sort, two passes", 3000000, 5000, 2, rng);
    check_sort("sort, three passes", 5000000, 5000, 3, rng);
    check_sort("sort, three passes at the link limit", 0xFFFFFFFEll, 5000, 3, rng);
    {
        const int64_t m = 5000000;
        const int64_t rowptr[3] = {0, 1234567, m};
        std::vector<int64_t> idx;
        for (int k = 0; k < 2000; ++k) idx.push_back((int64_t)k * 2477 + (k % 2 ? 3 : 0));
        std::shuffle(idx.begin(), idx.end(), rng);
        const RemovePlan p = remove_plan(2, rowptr, (int64_t)idx.size(), idx.data());
        std::vector<int64_t> asc(idx);
        std::sort(asc.begin(), asc.end());
        const int64_t before = std::lower_bound(asc.begin(), asc.end(), rowptr[1]) - asc.begin();
        if (p.verdict != REMOVE_OK || p.r != asc || p.rowptr_new != std::vector<int64_t>{0, rowptr[1] - before, m - 2000})
            fail("plan over 5 000 000 links");
    }
    // ---- every validation verdict with the entry it names
    {
        const std::vector<int64_t> deg = {3, 0, 4};           // m = 7
        check_verdict("valid", deg, {6, 0, 3}, 3, REMOVE_OK, -1);
        check_verdict("count 0 with an array", deg, {6, 0, 3}, 0, REMOVE_OK, -1);
        check_verdict("count 0 without one", deg, {}, 0, REMOVE_OK, -1);
        check_verdict("position m", deg, {1, 7, 2}, 3, REMOVE_BAD_RANGE, 1);
        check_verdict("negative position", deg, {-1, 2}, 2, REMOVE_BAD_RANGE, 0);
        check_verdict("two out of range: the first", deg, {2, 3, 99, -5}, 4, REMOVE_BAD_RANGE, 2);
        check_verdict("huge position", deg, {0, 1, 2, (int64_t)1 << 40}, 4, REMOVE_BAD_RANGE, 3);
        check_verdict("duplicate", deg, {4, 1, 4}, 3, REMOVE_DUPLICATE, 2);
        check_verdict("duplicate neighbours", deg, {5, 5}, 2, REMOVE_DUPLICATE, 1);
        check_verdict("three times: the second occurrence", deg, {2, 0, 2, 6, 2}, 5, REMOVE_DUPLICATE, 2);
        check_verdict("two duplicated values: the earlier second occurrence", deg, {6, 1, 3, 1, 6}, 5, REMOVE_DUPLICATE, 3);
        check_verdict("range comes before duplicate", deg, {1, 1, 7}, 3, REMOVE_BAD_RANGE, 2);
        check_verdict("no links: any position is out of range", {0, 0}, {0}, 1, REMOVE_BAD_RANGE, 0);
    }
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
