// Host-side check of the append plan (recommendersystems_amd/csrc/append_plan.h), built against the header alone by
// tests/test_append_plan.py: the plan of a few hundred small cases against a brute-force list-of-lists append
// (edges[src].Add(link), Graph.cs:40), then every validation verdict with the entry it reports.  Every case also goes through
// the kernels' own arithmetic (the ap_* functions of the header, which append.hip's k_append_rowptr and k_append_merge call):
// the new row pointers, and every chunk of old positions through BOTH paths of the merge, whichever the kernel would pick.
// Prints every failure and exits non-zero if there is one.
#include "append_plan.h"

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

// an old link is the pair (row, position in the row); an appended one (-1, q)
struct Tag { int64_t a, b; };
static bool same(const Tag &x, const Tag &y) { return x.a == y.a && x.b == y.b; }

// What the device does with the plan's tables.  rowptr_old has n_old + 1 entries (exactly: a read past them is the
// sanitizer's); the rows [n_old, n) are the call's new nodes.  want_rowptr: the brute-force append's row pointers.
static void check_kernel_arithmetic(const std::string &name, const AppendPlan &p, const std::vector<int64_t> &rowptr_old,
                                    int32_t n, const std::vector<int64_t> &want_rowptr)
{
    const int32_t n_old = (int32_t)rowptr_old.size() - 1;
    const int nb = (int)p.srcs.size();
    const int64_t m = p.m_old;
    // k_append_rowptr: one call per row pointer
    for (int64_t i = 0; i <= n; ++i)
        if (ap_rowptr_new(p.srcs.data(), p.cum.data(), nb, rowptr_old.data(), n_old, i) != want_rowptr[(size_t)i]) {
            fail(name + ": ap_rowptr_new(" + std::to_string(i) + ")");
            break;
        }
    // k_append_merge: every chunk through the dense and the sparse path
    std::vector<int64_t> dense((size_t)m, -1), sparse((size_t)m, -1);
    std::vector<int> written((size_t)p.m_new, 0);
    for (int64_t c0 = 0; c0 < m; c0 += AP_CHUNK) {
        const int64_t c1 = c0 + AP_CHUNK < m ? c0 + AP_CHUNK : m;
        const ApSlice s = ap_chunk_slice(p.brk.data(), nb, c0, c1);
        if (s.j < 0 || s.jend < s.j || s.jend > nb) { fail(name + ": chunk slice at " + std::to_string(c0)); return; }
        for (int k = 0; k < nb; ++k)
            if ((p.brk[(size_t)k] > c0 && p.brk[(size_t)k] <= c1 - 1) != (k >= s.j && k < s.jend)) {
                fail(name + ": breakpoint " + std::to_string(k) + " and the slice of chunk " + std::to_string(c0));
                break;
            }
        if (ap_chunk_dense(s) != (s.jend - s.j > 32)) fail(name + ": sparse / dense choice at " + std::to_string(c0));
        for (int64_t e = c0; e < c1; ++e) dense[(size_t)e] = ap_dense_dest(p.brk.data(), p.cum.data(), s, e);
        int j = s.j, segments = 0;
        for (int64_t a = c0; a < c1;) {
            const ApSeg g = ap_segment(p.brk.data(), p.cum.data(), nb, c1, a, j);
            if (g.a != a || g.b <= g.a || g.b > c1 || g.next < j || g.next > nb) {   // (never an empty segment: the walk ends)
                fail(name + ": segment at " + std::to_string(a) + " of chunk " + std::to_string(c0));
                return;
            }
            for (int64_t e = g.a; e < g.b; ++e) {
                if (sparse[(size_t)e] != -1) fail(name + ": the sparse path takes old position " + std::to_string(e) + " twice");
                sparse[(size_t)e] = e + g.sh;
            }
            a = g.b;
            j = g.next;
            ++segments;
        }
        if (segments > s.jend - s.j + 1) fail(name + ": more segments than breakpoints + 1 in chunk " + std::to_string(c0));
    }
    for (int64_t e = 0; e < m; ++e) {
        const int64_t want = e + p.shift(e);
        if (dense[(size_t)e] != want) { fail(name + ": dense path, old position " + std::to_string(e)); break; }
        if (sparse[(size_t)e] != want) { fail(name + ": sparse path, old position " + std::to_string(e)); break; }
        if (want < 0 || want >= p.m_new || written[(size_t)want]++) { fail(name + ": destination of " + std::to_string(e) + " taken"); break; }
    }
    for (size_t k = 0; k < p.pos.size(); ++k)
        if (p.pos[k] < 0 || p.pos[k] >= p.m_new || written[(size_t)p.pos[k]]++) {
            fail(name + ": an old link is merged onto the place of appended link " + std::to_string(k));
            break;
        }
}

// deg[i] links per row, the links (src[q], dst[q]) appended: checks every output of the plan against the lists.  The last
// n_new_rows rows (without links) are new nodes of the call: the device's old row pointers end before them.
static void check_case(const std::string &name, const std::vector<int64_t> &deg, const std::vector<int32_t> &src,
                       const std::vector<int32_t> &dst, int32_t n_new_rows = 0)
{
    const int32_t n = (int32_t)deg.size();
    const int64_t count = (int64_t)src.size();
    std::vector<int64_t> rowptr((size_t)n + 1, 0);
    for (int32_t i = 0; i < n; ++i) rowptr[(size_t)i + 1] = rowptr[i] + deg[i];
    const int64_t m = rowptr[n];

    // brute force: the lists, appended to, flattened again
    std::vector<std::vector<Tag>> lists((size_t)n);
    for (int32_t i = 0; i < n; ++i)
        for (int64_t e = 0; e < deg[i]; ++e) lists[i].push_back(Tag{i, e});
    for (int64_t q = 0; q < count; ++q) lists[(size_t)src[q]].push_back(Tag{-1, q});
    std::vector<Tag> flat;
    std::vector<int64_t> rowptr_new((size_t)n + 1, 0);
    for (int32_t i = 0; i < n; ++i) {
        for (const Tag &t : lists[i]) flat.push_back(t);
        rowptr_new[(size_t)i + 1] = (int64_t)flat.size();
    }

    const AppendPlan p = append_plan(n, rowptr.data(), count, src.data(), dst.data());
    if (p.verdict != APPEND_OK) { fail(name + ": verdict " + std::to_string((int)p.verdict)); return; }
    if (p.m_old != m || p.m_new != m + count) fail(name + ": m_old / m_new");
    if ((int64_t)p.order.size() != count || (int64_t)p.pos.size() != count || (int64_t)p.new_index.size() != count) {
        fail(name + ": table lengths");
        return;
    }
    check_kernel_arithmetic(name, p, std::vector<int64_t>(rowptr.begin(), rowptr.end() - n_new_rows), n, rowptr_new);
    const size_t D = p.srcs.size();
    if (p.cnt.size() != D || p.brk.size() != D || p.cum.size() != D) { fail(name + ": distinct-source table lengths"); return; }
    if ((int64_t)D > count) fail(name + ": more table entries than links");

    // the stable order by source
    for (int64_t k = 0; k + 1 < count; ++k) {
        const int64_t a = p.order[(size_t)k], b = p.order[(size_t)k + 1];
        if (src[a] > src[b] || (src[a] == src[b] && a > b)) fail(name + ": order is not stable by source at " + std::to_string(k));
    }
    std::vector<int> seen((size_t)count, 0);
    for (int64_t k = 0; k < count; ++k) {
        const int64_t q = p.order[(size_t)k];
        if (q < 0 || q >= count || seen[(size_t)q]++) { fail(name + ": order is no permutation"); return; }
    }
    // distinct sources with their counts, breakpoints and running sums
    int64_t run = 0;
    for (size_t j = 0; j < D; ++j) {
        if (j > 0 && p.srcs[j] <= p.srcs[j - 1]) fail(name + ": sources not strictly ascending");
        int64_t c = 0;
        for (int64_t q = 0; q < count; ++q) c += src[q] == p.srcs[j];
        if (c == 0 || c != p.cnt[j]) fail(name + ": count of source " + std::to_string(p.srcs[j]));
        run += p.cnt[j];
        if (p.cum[j] != run) fail(name + ": running sum " + std::to_string(j));
        if (p.brk[j] != rowptr[(size_t)p.srcs[j] + 1]) fail(name + ": breakpoint " + std::to_string(j));
        if (j > 0 && p.brk[j] < p.brk[j - 1]) fail(name + ": breakpoints decrease");
    }
    if (run != count) fail(name + ": counts do not add up");

    // every old link: position e of row i moves to e + shift(e), and shift(e) = appended links with src < i
    for (int32_t i = 0; i < n; ++i) {
        int64_t below = 0;
        for (int64_t q = 0; q < count; ++q) below += src[q] < i;
        if (p.row_shift(i) != below) fail(name + ": row_shift(" + std::to_string(i) + ")");
        if (rowptr[i] + p.row_shift(i) != rowptr_new[i]) fail(name + ": new row pointer " + std::to_string(i));
        for (int64_t e = rowptr[i]; e < rowptr[(size_t)i + 1]; ++e) {
            if (p.shift(e) != below) { fail(name + ": shift(" + std::to_string(e) + ") of row " + std::to_string(i)); continue; }
            const int64_t f = e + p.shift(e);
            if (f < 0 || f >= (int64_t)flat.size() || !same(flat[(size_t)f], Tag{i, e - rowptr[i]}))
                fail(name + ": old link " + std::to_string(e) + " lands on the wrong place");
        }
    }
    if (rowptr[n] + p.row_shift(n) != rowptr_new[n]) fail(name + ": new row pointer n");
    // every appended link
    for (int64_t q = 0; q < count; ++q) {
        const int64_t f = p.new_index[(size_t)q];
        if (f < 0 || f >= (int64_t)flat.size() || !same(flat[(size_t)f], Tag{-1, q}))
            fail(name + ": appended link " + std::to_string(q) + " lands on the wrong place");
    }
    for (int64_t k = 0; k < count; ++k)
        if (p.pos[(size_t)k] != p.new_index[(size_t)p.order[(size_t)k]]) fail(name + ": pos / new_index disagree");
    // old and new positions together cover [0, m + count) exactly once
    std::vector<int> hit((size_t)(m + count), 0);
    for (int64_t e = 0; e < m; ++e) {
        const int64_t f = e + p.shift(e);
        if (f >= 0 && f < m + count) ++hit[(size_t)f];
    }
    for (int64_t q = 0; q < count; ++q)
        if (p.new_index[(size_t)q] >= 0 && p.new_index[(size_t)q] < m + count) ++hit[(size_t)p.new_index[(size_t)q]];
    for (int64_t f = 0; f < m + count; ++f)
        if (hit[(size_t)f] != 1) { fail(name + ": new position " + std::to_string(f) + " written " + std::to_string(hit[(size_t)f]) + " times"); break; }
}

static long cases_checked = 0;

static void named_cases()
{
    // empty rows before, between and after the appended sources
    check_case("empty rows around", {0, 0, 3, 0, 0, 2, 0, 0}, {2, 5, 2}, {1, 1, 7});
    check_case("appends into empty rows", {0, 0, 3, 0, 0, 2, 0, 0}, {0, 4, 7, 3, 4}, {1, 2, 3, 4, 5});
    check_case("all rows empty", {0, 0, 0, 0, 0}, {3, 1, 3}, {0, 0, 0});
    // every link to one source
    check_case("one source", {2, 1, 4, 0, 3}, {2, 2, 2, 2, 2, 2}, {0, 1, 2, 3, 4, 0});
    // sources in descending order
    check_case("descending sources", {1, 2, 0, 3, 1, 2}, {5, 4, 3, 2, 1, 0}, {0, 0, 0, 0, 0, 0});
    // a source repeated non-adjacently
    check_case("repeated source", {1, 2, 0, 3, 1, 2}, {3, 1, 3, 5, 1, 3}, {0, 1, 2, 3, 4, 5});
    // count == 0
    check_case("count 0", {1, 2, 0, 3}, {}, {});
    // row 0 and row n-1
    check_case("row 0", {2, 2, 2}, {0}, {2});
    check_case("row n-1", {2, 2, 2}, {2}, {0});
    check_case("row 0 and row n-1", {0, 2, 0}, {2, 0, 2, 0}, {1, 1, 1, 1});
    check_case("one node", {3}, {0, 0}, {0, 0});
    cases_checked += 11;
}

// rows whose ends are the given old flat positions (non-decreasing; the last one is m_old)
static std::vector<int64_t> rows_ending_at(const std::vector<int64_t> &ends)
{
    std::vector<int64_t> deg(ends.size());
    for (size_t i = 0; i < ends.size(); ++i) deg[i] = ends[i] - (i ? ends[i - 1] : 0);
    return deg;
}
static std::vector<int32_t> zeros(size_t k) { return std::vector<int32_t>(k, 0); }

// The edges of the merge kernel's chunks (AP_CHUNK = 8 192 old positions) and of its sparse / dense choice (AP_DENSE_BREAKS =
// 32).  Appending to row s puts a breakpoint at the row's end, so the cases are written as row ends.
static void chunk_edge_cases()
{
    const int64_t C = AP_CHUNK;
    // list lengths around one and two chunks; breakpoints at 0 (an empty row 0), in the middle, at m - 1 and at m_old (the last
    // rows: no old link moves), every row appended to, then each one alone
    for (const int64_t m : {(int64_t)0, (int64_t)1, C - 1, C, C + 1, 2 * C + 1}) {
        const std::vector<int64_t> ends = {0, m / 3, m / 3, m > 0 ? m - 1 : 0, m, m};
        const std::vector<int64_t> deg = rows_ending_at(ends);
        const std::string name = "m_old " + std::to_string(m);
        check_case(name + ", every row", deg, {5, 0, 1, 2, 3, 4, 0, 4}, zeros(8));
        for (int32_t s = 0; s < 6; ++s) check_case(name + ", row " + std::to_string(s), deg, {s, s}, zeros(2));
        cases_checked += 7;
    }
    // a breakpoint exactly at a chunk's c0, at c1 - 1, at c1 (the next chunk's c0) and at m_old
    {
        const std::vector<int64_t> deg = rows_ending_at({C - 1, C, 2 * C - 1, 2 * C, 2 * C + 1});
        check_case("chunk edges, all", deg, {0, 1, 2, 3, 4}, zeros(5));
        for (int32_t s = 0; s < 5; ++s) check_case("chunk edges, row " + std::to_string(s), deg, {s}, zeros(1));
        check_case("chunk edges, c1 - 1 and c1", deg, {1, 0, 1}, zeros(3));
        cases_checked += 7;
    }
    // exactly 32 and exactly 33 distinct breakpoints inside one chunk: 33 in chunk 0 (dense) and 32 in chunk 1 (sparse), the
    // other way round, and 33 of which one sits on c0 and so counts for neither chunk
    for (int variant = 0; variant < 3; ++variant) {
        std::vector<int64_t> ends;
        std::vector<int32_t> src;
        const int n0 = variant == 1 ? 32 : 33, n1 = variant == 1 ? 33 : 32;
        for (int k = 0; k < n0; ++k) ends.push_back(100 + 200 * (int64_t)k);
        for (int k = 0; k < n1; ++k) ends.push_back(C + (variant == 2 ? 0 : 7) + 200 * (int64_t)k);
        ends.push_back(2 * C + 1);
        for (size_t i = 0; i + 1 < ends.size(); ++i) src.push_back((int32_t)i);
        src.push_back(3);
        check_case("32 / 33 breakpoints, variant " + std::to_string(variant), rows_ending_at(ends), src, zeros(src.size()));
        ++cases_checked;
    }
    // runs of coinciding breakpoints (sources that are neighbouring rows without links): a chunk in which ALL breakpoints
    // coincide, few enough for the sparse path and too many for it; runs among distinct ones; a run on c0 and one on m_old
    for (const int run : {3, 32, 33, 40}) {
        std::vector<int64_t> ends = {500};
        std::vector<int32_t> src;
        for (int k = 0; k < run; ++k) { ends.push_back(500); src.push_back((int32_t)k + 1); }
        ends.push_back(C + 5);
        check_case("all breakpoints coincide, run " + std::to_string(run), rows_ending_at(ends), src, zeros(src.size()));
        ends = {10, 10, 10, 700, 700, C, C, C, C + 9, 2 * C + 1, 2 * C + 1, 2 * C + 1};
        for (int k = 0; k < run; ++k) ends.insert(ends.begin() + 5, 700);
        src.clear();
        for (size_t i = 0; i < ends.size(); ++i) src.push_back((int32_t)(ends.size() - 1 - i));
        check_case("runs among distinct breakpoints, run " + std::to_string(run), rows_ending_at(ends), src, zeros(src.size()));
        cases_checked += 2;
    }
    // new nodes behind the last resident one: links from them, from the last resident row and from row 0
    for (const int64_t m : {(int64_t)0, C, C + 1}) {
        const std::vector<int64_t> deg = rows_ending_at({0, m / 2, m, m, m, m});
        check_case("new nodes, m_old " + std::to_string(m), deg, {5, 3, 2, 0, 4, 5, 1}, {4, 5, 3, 0, 0, 1, 5}, 3);
        check_case("new nodes without links from them, m_old " + std::to_string(m), deg, {1, 2}, {5, 4}, 3);
        check_case("new nodes alone, m_old " + std::to_string(m), deg, {}, {}, 3);
        cases_checked += 3;
    }
}

static void random_cases()
{
    std::mt19937_64 rng(20240611);
    for (int c = 0; c < 600; ++c) {
        const int32_t n = 1 + (int32_t)(rng() % 40);
        const int style = c % 6;
        std::vector<int64_t> deg((size_t)n);
        for (int32_t i = 0; i < n; ++i) {
            // (many empty rows in styles 1 and 4, so that breakpoints coincide)
            const bool empty = (style == 1 || style == 4) ? rng() % 3 != 0 : rng() % 5 == 0;
            deg[i] = empty ? 0 : 1 + (int64_t)(rng() % 6);
        }
        const int64_t count = style == 5 ? (int64_t)(rng() % 3) : (int64_t)(rng() % 60);
        std::vector<int32_t> src((size_t)count), dst((size_t)count);
        const int32_t one = (int32_t)(rng() % n);
        for (int64_t q = 0; q < count; ++q) {
            src[q] = style == 2 ? one : style == 3 ? (int32_t)((n - 1) - (q * n) / (count > 0 ? count : 1)) : (int32_t)(rng() % n);
            if (style == 4 && q % 7 == 0) src[q] = (q % 2) ? 0 : n - 1;
            dst[q] = (int32_t)(rng() % n);
        }
        check_case("random " + std::to_string(c) + " (style " + std::to_string(style) + ", n " + std::to_string(n) + ")", deg, src, dst);
        ++cases_checked;
    }
}

// The order by source is a radix sort of 11 bits a pass: node counts at which it takes one, two and three passes, and their
// boundaries, against std::stable_sort; the positions follow from the order (pos[k] = rowptr_old[source + 1] + k).
static void wide_cases()
{
    std::mt19937_64 rng(777);
    for (const int32_t n : {2047, 2048, 2049, 70000, (1 << 22) - 1, 1 << 22, (1 << 22) + 1, 5000000}) {
        for (int style = 0; style < 3; ++style) {
            const std::string name = "wide n " + std::to_string(n) + " style " + std::to_string(style);
            std::vector<int64_t> rowptr((size_t)n + 1, 0);
            for (int32_t i = 0; i < n; ++i) rowptr[(size_t)i + 1] = rowptr[i] + (int64_t)((i * 2654435761u >> 7) % 3);
            const int64_t count = style == 2 ? 5 : 3000;
            std::vector<int32_t> src((size_t)count), dst((size_t)count, 0);
            for (int64_t q = 0; q < count; ++q)   // (style 1: few sources, far apart, often repeated; the top node among them)
                src[q] = style == 1 ? (int32_t)((int64_t)(n - 1) - (int64_t)(rng() % 7) * ((n - 1) / 7)) : (int32_t)(rng() % (uint64_t)n);
            src[0] = n - 1;
            src[(size_t)count - 1] = 0;
            const AppendPlan p = append_plan(n, rowptr.data(), count, src.data(), dst.data());
            std::vector<int64_t> want((size_t)count);
            for (int64_t q = 0; q < count; ++q) want[q] = q;
            std::stable_sort(want.begin(), want.end(), [&](int64_t a, int64_t b) { return src[a] < src[b]; });
            if (p.verdict != APPEND_OK || p.order != want) { fail(name + ": order"); continue; }
            for (int64_t k = 0; k < count; ++k) {
                const int64_t q = want[k];
                if (p.pos[k] != rowptr[(size_t)src[q] + 1] + k || p.new_index[q] != p.pos[k]) { fail(name + ": position " + std::to_string(k)); break; }
                if (p.row_shift(src[q]) + (int64_t)0 > k) { fail(name + ": row_shift " + std::to_string(k)); break; }
            }
            if (p.cum.empty() || p.cum.back() != count || p.row_shift(n) != count) fail(name + ": running sums");
            ++cases_checked;
        }
    }
}

static void expect_verdict(const std::string &name, int32_t n, const std::vector<int64_t> &rowptr, const std::vector<int32_t> &src,
                           const std::vector<int32_t> &dst, AppendVerdict want, int64_t want_q)
{
    const AppendPlan p = append_plan(n, rowptr.data(), (int64_t)src.size(), src.data(), dst.data());
    if (p.verdict != want) fail(name + ": verdict " + std::to_string((int)p.verdict) + ", expected " + std::to_string((int)want));
    if (want != APPEND_OK && want != APPEND_TOO_MANY && p.bad_q != want_q)
        fail(name + ": reports entry " + std::to_string(p.bad_q) + ", expected " + std::to_string(want_q));
    if (want != APPEND_OK && (!p.order.empty() || !p.srcs.empty() || !p.new_index.empty())) fail(name + ": a refused call was planned");
    ++cases_checked;
}

static void verdicts()
{
    const std::vector<int64_t> rp = {0, 2, 2, 5, 6};   // n = 4
    expect_verdict("src -1", 4, rp, {0, -1, 2}, {0, 0, 0}, APPEND_BAD_SRC, 1);
    expect_verdict("src n", 4, rp, {0, 3, 4}, {0, 0, 0}, APPEND_BAD_SRC, 2);
    expect_verdict("src n at 0", 4, rp, {4}, {0}, APPEND_BAD_SRC, 0);
    expect_verdict("src INT32_MIN", 4, rp, {1, 1, 1, INT32_MIN}, {0, 0, 0, 0}, APPEND_BAD_SRC, 3);
    expect_verdict("first of two bad src", 4, rp, {0, 7, 9}, {0, 0, 0}, APPEND_BAD_SRC, 1);
    expect_verdict("dst -1", 4, rp, {0, 1, 2}, {-1, 0, 0}, APPEND_BAD_DST, 0);
    expect_verdict("dst n", 4, rp, {0, 1, 2}, {3, 3, 4}, APPEND_BAD_DST, 2);
    expect_verdict("dst INT32_MAX", 4, rp, {0, 1}, {0, INT32_MAX}, APPEND_BAD_DST, 1);
    expect_verdict("bad src wins over an earlier bad dst", 4, rp, {0, 1, 5}, {9, 0, 0}, APPEND_BAD_SRC, 2);
    expect_verdict("n-1 is in range", 4, rp, {3, 0}, {3, 0}, APPEND_OK, -1);
    // the link limit: nnz_raw + count <= 2^32 - 2
    const int64_t lim = APPEND_MAX_LINKS;
    if (lim != 4294967294ll) fail("the link limit is not 2^32-2");
    expect_verdict("limit reached exactly", 2, {0, lim - 2, lim - 2}, {0, 1}, {0, 0}, APPEND_OK, -1);
    expect_verdict("one past the limit", 2, {0, lim - 2, lim - 1}, {0, 1}, {0, 0}, APPEND_TOO_MANY, -1);
    expect_verdict("full graph", 2, {0, 5, lim}, {1}, {0}, APPEND_TOO_MANY, -1);
    expect_verdict("full graph, count 0", 2, {0, 5, lim}, {}, {}, APPEND_OK, -1);
    expect_verdict("bad src wins over the limit", 2, {0, 5, lim}, {2}, {0}, APPEND_BAD_SRC, 0);
    {   // positions beyond 2^31 are planned in 64 bits
        const std::vector<int64_t> big = {0, 3000000000ll, 3000000000ll, 4000000000ll};
        const std::vector<int32_t> s = {2, 0, 1}, d = {0, 0, 0};
        const AppendPlan p = append_plan(3, big.data(), 3, s.data(), d.data());
        if (p.verdict != APPEND_OK || p.new_index != std::vector<int64_t>{4000000002ll, 3000000000ll, 3000000001ll})
            fail("positions beyond 2^31");
        if (p.shift(2999999999ll) != 0 || p.shift(3000000000ll) != 2 || p.shift(3999999999ll) != 2) fail("shifts beyond 2^31");
        ++cases_checked;
    }
}

int main()
{
    named_cases();
    chunk_edge_cases();
    random_cases();
    wide_cases();
    verdicts();
    std::printf("%ld cases checked\n", cases_checked);
    std::printf("%d failures\n", failures);
    return failures != 0;
}
