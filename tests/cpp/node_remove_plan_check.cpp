// Host-side check of the node removal plan (recommendersystems_amd/csrc/node_remove_plan.h) and of what the device kernels of
// node_remove.hip compute with it (the nrm_* functions there, the very code the kernels compile), built against the header alone
// by tests/test_node_remove_plan.py.  Count, scan and scatter are replayed workgroup by workgroup, trip by trip and lane by
// lane, once in launch order and once backwards, through an element type that counts its reads and writes: every new link,
// every new row pointer, every entry of the per-link output and of the two ITEM orders written exactly once.  Every case is
// compared with a brute force: the lists of the removed nodes erased, the links to them erased, everything renumbered.
// Prints every failure and exits non-zero if there is one.
#include "node_remove_plan.h"

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

// an element that counts how often it is read and written
template <class T>
struct Counted {
    T val = T(-7);
    mutable int reads = 0;
    int writes = 0;
    void set(T v) { val = v; ++writes; }
    T get() const { ++reads; return val; }
};

struct Case {
    std::vector<std::vector<int32_t>> adj;   // targets per row, list order
    std::vector<uint8_t> is_item;
    std::vector<int64_t> id;
    std::vector<int32_t> rem;                // the call's node list
};

static Case make_case(int32_t n)
{
    Case c;
    c.adj.resize((size_t)n);
    c.is_item.assign((size_t)n, 0);
    c.id.resize((size_t)n);
    for (int32_t i = 0; i < n; ++i) { c.is_item[(size_t)i] = (uint8_t)(i % 3 != 0); c.id[(size_t)i] = 1000 + i; }
    return c;
}

// the ITEM rows by id descending, equal ids row-ascending: what rwr_graph_create's stable sort leaves
static std::vector<int32_t> item_order_of(const std::vector<uint8_t> &is_item, const std::vector<int64_t> &id)
{
    std::vector<int32_t> o;
    for (int32_t i = 0; i < (int32_t)is_item.size(); ++i)
        if (is_item[(size_t)i]) o.push_back(i);
    std::stable_sort(o.begin(), o.end(), [&](int32_t a, int32_t b) { return id[(size_t)a] > id[(size_t)b]; });
    return o;
}

struct Out {
    std::vector<Counted<int64_t>> w_n;       // carries the OLD position of the link
    std::vector<Counted<int32_t>> dst_n;
    std::vector<Counted<int64_t>> rp_n, link_out;
    std::vector<Counted<int32_t>> irows_n, iord_n;
    std::vector<int64_t> cnt, off;
};

// k_nrm_list_count / launch_cand_scan / k_nrm_list_scatter on the host
static void replay_list(const NodeRemovePlan &p, const std::vector<int32_t> &list, std::vector<Counted<int32_t>> &out, bool backwards)
{
    const int32_t len = (int32_t)list.size(), nb = nrm_list_blocks(len), n = p.n_old;
    std::vector<int32_t> off((size_t)nb + 1, 0);
    std::vector<std::vector<unsigned long long>> bal((size_t)nb, std::vector<unsigned long long>(NRM_WAVES, 0));
    for (int32_t b = 0; b < nb; ++b) {
        int c = 0;
        for (int t = 0; t < NRM_THREADS; ++t) {
            const int64_t q = (int64_t)b * NRM_THREADS + t;
            const int32_t row = q < len ? list[(size_t)q] : -1;
            const bool m = (uint32_t)row < (uint32_t)n && !nrm_removed(p.bits.data(), row);
            if (m) bal[(size_t)b][(size_t)(t / NRM_WAVE)] |= 1ull << (t % NRM_WAVE);
        }
        for (int q = 0; q < NRM_WAVES; ++q) c += nrm_wave_count(bal[(size_t)b][(size_t)q]);
        off[(size_t)b + 1] = c;
    }
    for (int32_t b = 0; b < nb; ++b) off[(size_t)b + 1] += off[(size_t)b];
    const int32_t total = p.n_items_new;
    if (nb > 0 && off[(size_t)nb] != total) fail("list compaction: the counts do not sum to n_items_new");
    for (int32_t bb = 0; bb < nb; ++bb) {
        const int32_t b = backwards ? nb - 1 - bb : bb;
        int wc[NRM_WAVES];
        for (int q = 0; q < NRM_WAVES; ++q) wc[q] = nrm_wave_count(bal[(size_t)b][(size_t)q]);
        for (int tt = 0; tt < NRM_THREADS; ++tt) {
            const int t = backwards ? NRM_THREADS - 1 - tt : tt;
            const int wv = t / NRM_WAVE, lane = t % NRM_WAVE;
            if (!((bal[(size_t)b][(size_t)wv] >> lane) & 1)) continue;
            const int pos = off[(size_t)b] + nrm_rank_in_chunk(0, wc, wv, bal[(size_t)b][(size_t)wv], lane);
            if (pos < 0 || pos >= total) { fail("list compaction: position outside [0, n_items_new)"); continue; }
            out[(size_t)pos].set(p.new_index[(size_t)list[(size_t)b * NRM_THREADS + (size_t)t]]);
        }
    }
}

// k_nrm_count, the scan (launch_cand_scan in 64 bits), k_nrm_scatter on the host
static Out replay(const NodeRemovePlan &p, const std::vector<int64_t> &rowptr, const std::vector<int32_t> &dst,
                  const std::vector<int32_t> &item_rows, const std::vector<int32_t> &item_order, bool backwards)
{
    const int32_t n = p.n_old;
    const int64_t m_old = p.m_old, m_cap = m_old - p.m_rows, nch = nrm_chunks(m_old), ni = (int64_t)p.iv_lo.size();
    const int64_t *lo = p.iv_lo.data(), *hi = p.iv_hi.data();
    const uint8_t *bits = p.bits.data();
    Out R;
    R.cnt.assign((size_t)nch, 0);
    for (int64_t cc = 0; cc < nch; ++cc) {
        const int64_t c = backwards ? nch - 1 - cc : cc;
        const int64_t c0 = c * NRM_CHUNK, c1 = std::min<int64_t>(c0 + NRM_CHUNK, m_old);
        const NrmSlice s = nrm_chunk_slice(lo, hi, ni, c0, c1);
        int64_t total = 0;
        for (int64_t t0 = c0; t0 < c1; t0 += NRM_THREADS)
            for (int wv = 0; wv < NRM_WAVES; ++wv) {
                unsigned long long bal = 0;
                for (int lane = 0; lane < NRM_WAVE; ++lane) {
                    const int64_t e = t0 + wv * NRM_WAVE + lane;
                    if (e < c1 && nrm_keep(lo, hi, s, bits, n, e, dst[(size_t)e])) bal |= 1ull << lane;
                }
                total += nrm_wave_count(bal);
            }
        R.cnt[(size_t)c] = total;
    }
    R.off.assign((size_t)nch + 1, 0);
    for (int64_t c = 0; c < nch; ++c) R.off[(size_t)c + 1] = R.off[(size_t)c] + R.cnt[(size_t)c];
    const int64_t m_new = R.off[(size_t)nch];
    if (m_new > m_cap) fail("more kept links than the link buffers hold");
    R.w_n.resize((size_t)std::max<int64_t>(m_cap, 1));
    R.dst_n.resize((size_t)std::max<int64_t>(m_cap, 1));
    R.rp_n.resize((size_t)p.n_new + 1);
    R.link_out.resize((size_t)std::max<int64_t>(m_old, 1));
    for (int64_t cc = 0; cc < nch; ++cc) {
        const int64_t c = backwards ? nch - 1 - cc : cc;
        const int64_t c0 = c * NRM_CHUNK, c1 = std::min<int64_t>(c0 + NRM_CHUNK, m_old);
        const NrmSlice s = nrm_chunk_slice(lo, hi, ni, c0, c1);
        const int64_t o = R.off[(size_t)c];
        std::vector<uint16_t> pre((size_t)NRM_CHUNK + 1, 0xFFFF);
        int base = 0;
        for (int64_t t0 = c0; t0 < c1; t0 += NRM_THREADS) {
            unsigned long long bal[NRM_WAVES];
            int wc[NRM_WAVES];
            for (int wv = 0; wv < NRM_WAVES; ++wv) {
                bal[wv] = 0;
                for (int lane = 0; lane < NRM_WAVE; ++lane) {
                    const int64_t e = t0 + wv * NRM_WAVE + lane;
                    if (e < c1 && nrm_keep(lo, hi, s, bits, n, e, dst[(size_t)e])) bal[wv] |= 1ull << lane;
                }
                wc[wv] = nrm_wave_count(bal[wv]);
            }
            for (int tt = 0; tt < NRM_THREADS; ++tt) {
                const int t = backwards ? NRM_THREADS - 1 - tt : tt;
                const int wv = t / NRM_WAVE, lane = t % NRM_WAVE;
                const int64_t e = t0 + t;
                if (e >= c1) continue;
                const bool k = (bal[wv] >> lane) & 1;
                const int rank = nrm_rank_in_chunk(base, wc, wv, bal[wv], lane);
                pre[(size_t)(e - c0)] = (uint16_t)rank;
                const int64_t to = o + rank;
                if (k) {
                    if (to < 0 || to >= m_new) { fail("kept link outside [0, m_new)"); continue; }
                    R.w_n[(size_t)to].set(e);
                    R.dst_n[(size_t)to].set(p.new_index[(size_t)dst[(size_t)e]]);
                }
                R.link_out[(size_t)e].set(k ? to : -1);
            }
            for (int wv = 0; wv < NRM_WAVES; ++wv) base += wc[wv];
        }
        pre[(size_t)(c1 - c0)] = (uint16_t)base;
        const NrmRows rows = nrm_chunk_rows(rowptr.data(), n, c0, c1, c + 1 == nch);
        for (int64_t ii = rows.lo; ii < rows.hi; ++ii) {
            const int64_t i = backwards ? rows.hi - 1 - (ii - rows.lo) : ii;
            const int32_t to = p.new_index[(size_t)i];
            if (to < 0) continue;
            const int64_t at = rowptr[(size_t)i] - c0;
            if (at < 0 || at > c1 - c0 || pre[(size_t)at] == 0xFFFF) { fail("row start outside its chunk's prefix table"); continue; }
            R.rp_n[(size_t)to].set(o + pre[(size_t)at]);
        }
    }
    R.irows_n.resize((size_t)std::max(p.n_items_new, 1));
    R.iord_n.resize((size_t)std::max(p.n_items_new, 1));
    replay_list(p, item_rows, R.irows_n, backwards);
    replay_list(p, item_order, R.iord_n, backwards);
    return R;
}

static void check_case(const std::string &name, const Case &c)
{
    const int32_t n = (int32_t)c.adj.size(), count = (int32_t)c.rem.size();
    std::vector<int64_t> rowptr((size_t)n + 1, 0);
    std::vector<int32_t> dst;
    for (int32_t i = 0; i < n; ++i) {
        for (int32_t d : c.adj[(size_t)i]) dst.push_back(d);
        rowptr[(size_t)i + 1] = (int64_t)dst.size();
    }
    const int64_t m = rowptr[(size_t)n];
    // ---- brute force
    std::vector<uint8_t> gone((size_t)n, 0);
    for (int32_t r : c.rem) gone[(size_t)r] = 1;
    std::vector<int32_t> nidx((size_t)n, -1);
    int32_t n_new = 0;
    for (int32_t i = 0; i < n; ++i)
        if (!gone[(size_t)i]) nidx[(size_t)i] = n_new++;
    std::vector<int64_t> rp_new{0}, kept_old;
    std::vector<int32_t> dst_new;
    std::vector<int64_t> lidx((size_t)m, -1);
    std::vector<uint8_t> item_new;
    std::vector<int64_t> id_new;
    for (int32_t i = 0; i < n; ++i) {
        if (gone[(size_t)i]) continue;
        for (int64_t e = rowptr[(size_t)i]; e < rowptr[(size_t)i + 1]; ++e)
            if (!gone[(size_t)dst[(size_t)e]]) {
                lidx[(size_t)e] = (int64_t)kept_old.size();
                kept_old.push_back(e);
                dst_new.push_back(nidx[(size_t)dst[(size_t)e]]);
            }
        rp_new.push_back((int64_t)kept_old.size());
        item_new.push_back(c.is_item[(size_t)i]);
        id_new.push_back(c.id[(size_t)i]);
    }
    const int64_t m_new = (int64_t)kept_old.size();
    std::vector<int32_t> irows_new;
    for (int32_t i = 0; i < n_new; ++i)
        if (item_new[(size_t)i]) irows_new.push_back(i);
    const std::vector<int32_t> iord_new = item_order_of(item_new, id_new);

    // ---- the plan
    const NodeRemovePlan p = node_remove_plan(n, rowptr.data(), c.is_item.data(), count, c.rem.data());
    if (p.verdict != NODE_REMOVE_OK) { fail(name + ": verdict " + std::to_string((int)p.verdict)); return; }
    if (p.n_old != n || p.n_new != n_new || p.m_old != m) fail(name + ": n_old / n_new / m_old");
    if ((int32_t)p.new_index.size() != n + 1 || p.new_index[(size_t)n] != n_new) fail(name + ": new_index size or end");
    for (int32_t i = 0; i < n; ++i)
        if (p.new_index[(size_t)i] != nidx[(size_t)i] || nrm_removed(p.bits.data(), i) != (gone[(size_t)i] != 0)) { fail(name + ": new_index / bitmap at " + std::to_string(i)); break; }
    if (p.is_item_new != item_new || p.n_items_new != (int32_t)irows_new.size()) fail(name + ": is_item_new / n_items_new");
    int64_t rows_links = 0;
    std::vector<uint8_t> in_iv((size_t)m, 0);
    for (size_t k = 0; k < p.iv_lo.size(); ++k) {
        if (p.iv_lo[k] >= p.iv_hi[k]) fail(name + ": an empty interval");
        if (k > 0 && p.iv_lo[k] < p.iv_hi[k - 1]) fail(name + ": intervals overlap or are not sorted");
        for (int64_t e = p.iv_lo[k]; e < p.iv_hi[k]; ++e) in_iv[(size_t)e] = 1;
        rows_links += p.iv_hi[k] - p.iv_lo[k];
    }
    if (rows_links != p.m_rows) fail(name + ": m_rows");
    for (int32_t i = 0; i < n; ++i)
        for (int64_t e = rowptr[(size_t)i]; e < rowptr[(size_t)i + 1]; ++e)
            if ((in_iv[(size_t)e] != 0) != (gone[(size_t)i] != 0)) { fail(name + ": intervals are not the removed rows"); i = n; break; }

    // ---- the replay, forwards and backwards
    const std::vector<int32_t> iord_old = item_order_of(c.is_item, c.id);
    std::vector<int32_t> irows_old;
    for (int32_t i = 0; i < n; ++i)
        if (c.is_item[(size_t)i]) irows_old.push_back(i);
    for (int pass = 0; pass < 2; ++pass) {
        const std::string nm = name + (pass ? " (backwards)" : "");
        const Out R = replay(p, rowptr, dst, irows_old, iord_old, pass == 1);
        if (R.off.back() != m_new) { fail(nm + ": m_new"); continue; }
        bool ok = true;
        for (int64_t q = 0; q < m_new && ok; ++q) {
            if (R.w_n[(size_t)q].writes != 1 || R.dst_n[(size_t)q].writes != 1) { fail(nm + ": new position " + std::to_string(q) + " not written exactly once"); ok = false; }
            else if (R.w_n[(size_t)q].val != kept_old[(size_t)q] || R.dst_n[(size_t)q].val != dst_new[(size_t)q]) { fail(nm + ": link at new position " + std::to_string(q)); ok = false; }
        }
        for (size_t q = (size_t)m_new; q < R.w_n.size(); ++q)
            if (R.w_n[q].writes != 0) { fail(nm + ": a write behind m_new"); break; }
        for (int32_t i = 0; i <= n_new; ++i) {
            if (R.rp_n[(size_t)i].writes != 1) { fail(nm + ": row pointer " + std::to_string(i) + " written " + std::to_string(R.rp_n[(size_t)i].writes) + " times"); break; }
            if (R.rp_n[(size_t)i].val != rp_new[(size_t)i]) { fail(nm + ": row pointer " + std::to_string(i)); break; }
        }
        for (int64_t e = 0; e < m; ++e) {
            if (R.link_out[(size_t)e].writes != 1) { fail(nm + ": link output not written exactly once"); break; }
            if (R.link_out[(size_t)e].val != lidx[(size_t)e]) { fail(nm + ": link output at " + std::to_string(e)); break; }
        }
        for (size_t q = 0; q < irows_new.size(); ++q) {
            if (R.irows_n[q].writes != 1 || R.iord_n[q].writes != 1) { fail(nm + ": ITEM order entry not written exactly once"); break; }
            if (R.irows_n[q].val != irows_new[q]) { fail(nm + ": item_rows at " + std::to_string(q)); break; }
            if (R.iord_n[q].val != iord_new[q]) { fail(nm + ": item_order at " + std::to_string(q)); break; }
        }
    }
}

static void check_verdicts()
{
    const int64_t rp[5] = {0, 2, 2, 5, 6};
    const uint8_t it[4] = {0, 1, 1, 0};
    auto run = [&](std::vector<int32_t> v) { return node_remove_plan(4, rp, it, (int32_t)v.size(), v.data()); };
    NodeRemovePlan p = run({1, 4, -1, 1});
    if (p.verdict != NODE_REMOVE_BAD_RANGE || p.bad_q != 1) fail("verdict: the first index out of range");
    p = run({1, -1});
    if (p.verdict != NODE_REMOVE_BAD_RANGE || p.bad_q != 1) fail("verdict: a negative index");
    p = run({3, 1, 2, 1, 3});
    if (p.verdict != NODE_REMOVE_DUPLICATE || p.bad_q != 3) fail("verdict: the second occurrence of the first repeat");
    p = run({2, 2, 9});
    if (p.verdict != NODE_REMOVE_BAD_RANGE || p.bad_q != 2) fail("verdict: range comes before duplicate");
    p = run({0, 0, 1, 2});
    if (p.verdict != NODE_REMOVE_DUPLICATE || p.bad_q != 1) fail("verdict: duplicate comes before count == n");
    p = run({3, 0, 2, 1});
    if (p.verdict != NODE_REMOVE_ALL) fail("verdict: count == n");
    p = run({});
    if (p.verdict != NODE_REMOVE_OK || p.n_new != 4 || p.m_rows != 0 || !p.iv_lo.empty()) fail("verdict: count == 0");
    p = node_remove_plan(4, rp, it, -3, nullptr);
    if (p.verdict != NODE_REMOVE_OK || p.n_new != 4) fail("verdict: a negative count plans nothing");
}

int main()
{
    check_verdicts();
    std::mt19937_64 rng(20241);
    auto rnd = [&](int64_t a, int64_t b) { return (int64_t)(a + (int64_t)(rng() % (uint64_t)(b - a + 1))); };
    {   // count == 0: everything stays, through the same replay
        Case c = make_case(40);
        for (int32_t i = 0; i < 40; ++i)
            for (int k = 0; k < i % 5; ++k) c.adj[(size_t)i].push_back((int32_t)rnd(0, 39));
        check_case("count 0", c);
        c.rem = {0, 39};
        check_case("node 0 and node n - 1", c);
        c.rem = {39, 0, 20};
        check_case("node 0, n - 1 and one in between, unsorted", c);
    }
    {   // a node without links, in or out
        Case c = make_case(12);
        for (int32_t i = 0; i < 12; ++i)
            if (i != 5) c.adj[(size_t)i] = {(int32_t)((i + 1) % 12 == 5 ? 6 : (i + 1) % 12), 0};
        c.rem = {5};
        check_case("a node without links", c);
        Case g = make_case(3);   // a graph without any link
        g.rem = {1};
        check_case("a graph without links", g);
    }
    {   // a removed row across the chunk edge: positions 8 190 .. 8 194
        Case c = make_case(300);
        for (int k = 0; k < 8190; ++k) c.adj[0].push_back((int32_t)rnd(2, 299));
        for (int k = 0; k < 5; ++k) c.adj[1].push_back((int32_t)rnd(2, 299));
        for (int32_t i = 2; i < 300; ++i)
            for (int k = 0; k < i % 7; ++k) c.adj[(size_t)i].push_back((int32_t)rnd(0, 299));
        c.rem = {1};
        check_case("a removed row across positions 8 190 .. 8 194", c);
        c.rem = {1, 0};
        check_case("the first chunk removed whole by its rows", c);
    }
    {   // a removed target whose in-links fill a whole chunk: that chunk keeps nothing, and 8 192 rows start in it
        const int32_t n = 8192 + 50;
        Case c = make_case(n);
        const int32_t hub = n - 1;
        for (int32_t i = 0; i < 8192; ++i) c.adj[(size_t)i] = {hub};
        for (int32_t i = 8192; i < n - 1; ++i) c.adj[(size_t)i] = {(int32_t)rnd(0, n - 2), hub, (int32_t)rnd(0, n - 2)};
        c.rem = {hub};
        check_case("a hub target: one chunk keeps nothing", c);
        c.rem = {hub, 17, 18, 8191, 8192};
        check_case("a hub target and rows at the chunk edge", c);
    }
    {   // consecutive removed rows, empty rows around and between them, trailing empty rows
        Case c = make_case(16);
        const int deg[16] = {2, 0, 3, 4, 0, 0, 1, 5, 0, 2, 0, 0, 3, 0, 0, 0};
        for (int32_t i = 0; i < 16; ++i)
            for (int k = 0; k < deg[i]; ++k) c.adj[(size_t)i].push_back((int32_t)rnd(0, 15));
        c.rem = {2, 3, 4, 6, 7, 8};
        check_case("consecutive removed rows and empty rows", c);
        c.rem = {1, 5, 10, 13, 15};
        check_case("only empty rows removed", c);
        c.rem = {12, 13, 14, 15};
        check_case("the trailing rows removed", c);
        c.rem.clear();
        for (int32_t i = 0; i < 16; ++i)
            if (i != 7) c.rem.push_back(i);
        check_case("every node but one", c);
        c.adj[7] = {7, 7};
        check_case("every node but one, which links to itself", c);
    }
    {   // a short last chunk and a full one
        Case c = make_case(64);
        for (int k = 0; k < 8192 + 3; ++k) c.adj[(size_t)rnd(0, 63)].push_back((int32_t)rnd(0, 63));
        c.rem = {3, 40, 63};
        check_case("a short last chunk", c);
        Case d = make_case(64);
        for (int k = 0; k < 2 * 8192; ++k) d.adj[(size_t)rnd(0, 63)].push_back((int32_t)rnd(0, 63));
        d.rem = {0, 31};
        check_case("two full chunks", d);
    }
    {   // equal ITEM ids on both sides of a removed ITEM row: the order among them stays row-ascending
        Case c = make_case(600);
        for (int32_t i = 0; i < 600; ++i) { c.is_item[(size_t)i] = 1; c.id[(size_t)i] = 50 + (i % 4 == 0 ? 0 : i % 3); }
        for (int32_t i = 0; i < 600; ++i) c.adj[(size_t)i] = {(int32_t)rnd(0, 599)};
        c.rem = {4, 5, 6, 255, 256, 257, 300};
        check_case("equal ITEM ids across removed rows", c);
        c.rem.clear();
        for (int32_t i = 0; i < 600; ++i)
            if (c.id[(size_t)i] == 52) c.rem.push_back(i);
        check_case("the largest ITEM id removed", c);
        for (int32_t i = 0; i < 600; ++i) c.is_item[(size_t)i] = (uint8_t)(i == 77);
        c.rem = {77};
        check_case("the last ITEM removed", c);
    }
    for (int it = 0; it < 300; ++it) {
        const int32_t n = (int32_t)rnd(1, 70);
        Case c = make_case(n);
        for (int32_t i = 0; i < n; ++i) {
            c.is_item[(size_t)i] = (uint8_t)rnd(0, 1);
            c.id[(size_t)i] = rnd(-5, 12);
            const int64_t d = rnd(0, 3) == 0 ? 0 : rnd(0, 9);
            for (int64_t k = 0; k < d; ++k) c.adj[(size_t)i].push_back((int32_t)rnd(0, n - 1));
        }
        std::vector<int32_t> perm((size_t)n);
        for (int32_t i = 0; i < n; ++i) perm[(size_t)i] = i;
        std::shuffle(perm.begin(), perm.end(), rng);
        perm.resize((size_t)rnd(0, n - 1));
        c.rem = perm;
        check_case("random " + std::to_string(it), c);
    }
    for (int it = 0; it < 12; ++it) {   // ... and with several chunks
        const int32_t n = (int32_t)rnd(150, 400);
        Case c = make_case(n);
        for (int32_t i = 0; i < n; ++i) {
            c.is_item[(size_t)i] = (uint8_t)rnd(0, 1);
            c.id[(size_t)i] = rnd(0, 40);
            const int64_t d = rnd(0, 4) == 0 ? 0 : rnd(0, 150);
            for (int64_t k = 0; k < d; ++k) c.adj[(size_t)i].push_back((int32_t)(rnd(0, 3) == 0 ? 7 : rnd(0, n - 1)));
        }
        std::vector<int32_t> perm((size_t)n);
        for (int32_t i = 0; i < n; ++i) perm[(size_t)i] = i;
        std::shuffle(perm.begin(), perm.end(), rng);
        perm.resize((size_t)rnd(1, n / 3));
        if (it % 2 == 0 && std::find(perm.begin(), perm.end(), 7) == perm.end()) perm.push_back(7);
        c.rem = perm;
        check_case("random, several chunks " + std::to_string(it), c);
    }
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
