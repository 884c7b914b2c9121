// rwr_graph_append_links / rwr_graph_append_nodes: links appended to the lists of a resident graph, and
// nodes appended behind its last one.  The host plans (append_plan.h, node_append_plan.h) say where everything goes; the kernels
// here merge the resident raw lists with the new links, and the resident ITEM order with the new ITEM rows, into NEW buffers, the
// handle takes them, and build.hip's re-derive (the incremental rebuild with nothing to patch) rebuilds the walk's data from
// them -- the same kernels in the same order as rwr_graph_create, hence the same bits.
#include "engine.h"
#include "append_plan.h"
#include "node_append_plan.h"
#include "seg_copy.h"

#include <chrono>
#include <cstdio>
#include <cstring>
#include <vector>

namespace rwr {

// ---- rwr_graph_append_links: the resident raw lists merged with a few new links, on the device.
// The host plan (append_plan.h) leaves one table entry per DISTINCT appended source s_j: brk[j] = rowptr_old[s_j + 1] and
// cum[j] = links appended to s_0 .. s_j.  The old flat position e moves to e + cum[upper_bound(brk, e) - 1]: between two
// breakpoints the move is constant, so the copy is a sequence of plain shifted block copies.
constexpr int AP_THREADS = SEG_THREADS;   // (seg_copy.h: the lanes of a segment's block copies)
constexpr int AP_CHUNK = 8192;     // old positions per workgroup
// More breakpoints than this in a chunk: the dense path of k_append_merge (per-element shifts).  The value is reasoned, not
// tuned: a segment is walked by all 256 lanes, so segments under 256 elements leave lanes idle in every one of the three block
// copies, and 8 192 / 32 = 256 is the average segment length at which that starts.  A bisection over at most 8 192 breakpoints
// of the chunk costs each element up to 13 uniform-ish loads from a table the whole workgroup keeps in cache.
constexpr int AP_DENSE_BREAKS = 32;

// the experiments build's wall-clock stamps (RWR_APPEND_TIMING=1), as RWR_BUILD_TIMING in build.h: tools/append_latency.py
static double at_now()
{
    using namespace std::chrono;
    return duration<double, std::micro>(steady_clock::now().time_since_epoch()).count();
}
static const bool at_on = [] { const char *e = RWR_TUNE_ENV("RWR_APPEND_TIMING"); return e && atoi(e) != 0; }();
#define AT(label) do { if (at_on) { const double t__ = at_now(); fprintf(stderr, "[append] %-28s %8.1f us\n", label, t__ - at_t); at_t = t__; } } while (0)

// rowptr_new[i] = rowptr_old[min(i, n_old)] + (appended links with src < i), i in [0, n]: the rows past n_old are the call's
// new nodes, whose lists were empty before it
__global__ __launch_bounds__(256) void k_append_rowptr(int32_t n, int32_t n_old, int32_t nb, const int32_t *__restrict__ srcs,
                                                       const int64_t *__restrict__ cum, const int64_t *__restrict__ rp_old,
                                                       int64_t *__restrict__ rp_new)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    int lo = 0, hi = nb;               // lower_bound(srcs, i)
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((int64_t)srcs[mid] < i) lo = mid + 1;
        else hi = mid;
    }
    rp_new[i] = rp_old[i < n_old ? i : (int64_t)n_old] + (lo > 0 ? cum[lo - 1] : 0);
}

// A workgroup takes AP_CHUNK consecutive old positions and finds the breakpoints inside its chunk ONCE, brk[j .. jend) (every
// lane runs the same two bisections: uniform loads).  Then one of two paths, chosen per chunk:
// * sparse, at most AP_DENSE_BREAKS breakpoints in the chunk: it walks them, and each segment in between is three shifted
//   block copies without any search per element;
// * dense, more than that: every lane takes elements in lane order and finds each one's shift by bisecting brk[j .. jend).
// Both write every old position of the chunk exactly once, at e + shift(e): the choice changes the speed, never the result.
__global__ __launch_bounds__(AP_THREADS) void k_append_merge(int64_t m_old, int32_t nb, const int64_t *__restrict__ brk,
                                                             const int64_t *__restrict__ cum, const int32_t *__restrict__ dst_o,
                                                             const uint8_t *__restrict__ et_o, const double *__restrict__ w_o,
                                                             int32_t *__restrict__ dst_n, uint8_t *__restrict__ et_n,
                                                             double *__restrict__ w_n)
{
    const int tid = threadIdx.x;
    const int64_t c0 = (int64_t)blockIdx.x * AP_CHUNK;
    const int64_t c1 = c0 + AP_CHUNK < m_old ? c0 + AP_CHUNK : m_old;
    int lo = 0, hi = nb;               // upper_bound(brk, c0)
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (brk[mid] <= c0) lo = mid + 1;
        else hi = mid;
    }
    int j = lo;
    // Many breakpoints inside the chunk (a bulk append that touches most rows: segments of a few dozen elements, which would
    // leave most lanes idle in the block copies below): every lane takes elements of the chunk in lane order and finds each
    // one's shift by bisecting the chunk's OWN breakpoints, brk[j .. jend) -- at most 13 steps over entries the whole workgroup
    // reads.  brk[0 .. j) <= c0 <= e, so the bisection of [j, jend) is the global upper_bound(brk, e).  Loads stay
    // lane-consecutive; the stores of a wave fall into a few pieces of consecutive addresses.
    int jend = j;
    {
        int h2 = nb;                   // upper_bound(brk, c1 - 1) within [j, nb)
        while (jend < h2) {
            const int mid = (jend + h2) >> 1;
            if (brk[mid] <= c1 - 1) jend = mid + 1;
            else h2 = mid;
        }
    }
    if (jend - j > AP_DENSE_BREAKS) {
        for (int64_t e = c0 + tid; e < c1; e += AP_THREADS) {
            int l2 = j, h2 = jend;     // upper_bound(brk, e) within [j, jend)
            while (l2 < h2) {
                const int mid = (l2 + h2) >> 1;
                if (brk[mid] <= e) l2 = mid + 1;
                else h2 = mid;
            }
            const int64_t sh = l2 > 0 ? cum[l2 - 1] : 0;
            w_n[e + sh] = w_o[e];
            dst_n[e + sh] = dst_o[e];
            et_n[e + sh] = et_o[e];
        }
        return;
    }
    int64_t a = c0;
    while (a < c1) {
        const int64_t sh = j > 0 ? cum[j - 1] : 0;             // (brk[j] > a here)
        const int64_t b = (j < nb && brk[j] < c1) ? brk[j] : c1;
        copy_seg<double>(w_o, w_n, a, b, sh, tid);
        copy_seg<int32_t>(dst_o, dst_n, a, b, sh, tid);
        copy_seg_bytes(et_o, et_n, a, b, sh, tid);
        a = b;
        while (j < nb && brk[j] <= a) ++j;                      // (coinciding breakpoints: rows without links in between)
    }
}

// the new links into the gaps the merge left: pos[k] ascending (the links are in list order)
__global__ __launch_bounds__(256) void k_append_scatter(int64_t count, const int64_t *__restrict__ pos, const int32_t *__restrict__ dst_a,
                                                        const uint8_t *__restrict__ et_a, const double *__restrict__ w_a,
                                                        int32_t *__restrict__ dst_n, uint8_t *__restrict__ et_n,
                                                        double *__restrict__ w_n)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= count) return;
    const int64_t p = pos[k];
    dst_n[p] = dst_a[k];
    et_n[p] = et_a[k];
    w_n[p] = w_a[k];
}

// ---- rwr_graph_append_nodes: the resident ITEM order (ids descending) merged with the call's new ITEM rows.
// A = the resident item_order, B = the new ITEM rows stably by id descending (node_append_plan.h, which also states the tie
// rule: A wins).  One thread per output element; its destination is its own position plus the elements of the OTHER list that
// stand before it, found by one bisection there.  Every destination in [0, no + nn) is written exactly once.
__global__ __launch_bounds__(256) void k_item_order_merge(int32_t no, int32_t nn, const int32_t *__restrict__ A,
                                                          const int32_t *__restrict__ B, const int64_t *__restrict__ node_id,
                                                          int32_t *__restrict__ out)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)no + nn) return;
    if (t < no) {
        const int32_t q = (int32_t)t, row = A[q];
        out[nap_old_dest(q, node_id[row], nn, [&](int32_t r) { return node_id[B[r]]; })] = row;
    } else {
        const int32_t r = (int32_t)(t - no), row = B[r];
        out[nap_new_dest(r, node_id[row], no, [&](int32_t q) { return node_id[A[q]]; })] = row;
    }
}

// the host row pointers of a call that adds nodes are grown BEFORE the link plan reads them; a call that fails before the swap
// gives the added entries back
struct RowptrGrowth {
    std::vector<int64_t> &rp;
    size_t old_size;
    bool keep = false;
    ~RowptrGrowth() { if (!keep) rp.resize(old_size); }
};

// Appends nodes and links to the resident raw lists and re-derives (rwr_graph_append_links; rwr_graph_append_nodes,
// §3.13).  Two phases: everything up to the swap works on NEW buffers -- an argument error or a failed allocation leaves the
// graph as it was -- and from the swap on (*swapped) a failure leaves raw and derived arrays out of step, as in
// graph_update_links.  With n_new == 0 this is the links-only append, launch for launch.
int32_t graph_append(rwr_graph *g, const char *who, int32_t n_new, const int64_t *node_id, const uint8_t *node_type,
                     int64_t count, const int32_t *src, const int32_t *dst, const uint8_t *etype, const double *w,
                     int64_t *new_index_out, bool *swapped)
{
    const int32_t n_old = g->n;
    hipStream_t s = g->stream;
    *swapped = false;
    double at_t = at_on ? at_now() : 0.0;
    const NodeAppendPlan np = node_append_plan(n_old, n_new, node_id, node_type, (uint8_t)RWR_NODE_ITEM);
    if (np.verdict == NODE_APPEND_TOO_MANY) {
        set_error("%s: %d + %d nodes exceed this build's limit of 2^31-1", who, n_old, n_new);
        return RWR_E_UNSUPPORTED;
    }
    const int32_t n = np.n_total;
    const bool grow = n > n_old;
    RowptrGrowth growth{g->h_rowptr, g->h_rowptr.size()};
    if (grow) {
        g->h_is_item.reserve((size_t)n);                        // (so that nothing on the host can fail after the swap)
        node_append_extend_rowptr(g->h_rowptr, n_old, n);
    }
    const AppendPlan plan = append_plan(n, g->h_rowptr.data(), count, src, dst);
    if (plan.verdict == APPEND_BAD_SRC) {
        set_error("%s: src[%lld] = %d is outside [0, %d)", who, (long long)plan.bad_q, src[plan.bad_q], n);
        return RWR_E_RANGE;
    }
    if (plan.verdict == APPEND_BAD_DST) {
        set_error("%s: dst[%lld] = %d is outside [0, %d)", who, (long long)plan.bad_q, dst[plan.bad_q], n);
        return RWR_E_RANGE;
    }
    if (plan.verdict == APPEND_TOO_MANY) {
        set_error("%s: %lld + %lld links exceed this build's per-device limit of 2^32-2", who, (long long)plan.m_old,
                  (long long)count);
        return RWR_E_UNSUPPORTED;
    }
    if (count <= 0 && !grow) {
        *swapped = true;               // (nothing to merge: a plain rebuild, with rwr_graph_update_links' failure rule)
        return graph_update_links(g, 0, nullptr, nullptr, nullptr);
    }
    const bool links = count > 0;
    const int64_t m_old = plan.m_old, m_new = plan.m_new;
    const size_t nb = plan.srcs.size();
    const int32_t ni_old = g->n_items, ni_new = np.n_new_items, ni = ni_old + ni_new;
    AT("plan (host)");
    // the new links in list order
    std::vector<int32_t> h_dst((size_t)(links ? count : 0));
    std::vector<uint8_t> h_et((size_t)(links ? count : 0));
    std::vector<double> h_w((size_t)(links ? count : 0));
    for (int64_t k = 0; k < count; ++k) {
        const int64_t q = plan.order[(size_t)k];
        h_dst[(size_t)k] = dst[q];
        h_et[(size_t)k] = etype[q];
        h_w[(size_t)k] = w[q];
    }
    AT("new links in order (host)");
    // ---- phase 1: every buffer exists before anything is launched
    DevBuf<int64_t> rp_n, d_brk, d_cum, d_pos;
    DevBuf<int32_t> dst_n, d_srcs, d_dst;
    DevBuf<uint8_t> et_n, d_et;
    DevBuf<double> w_n, wn_n, d_w;
    RWR_TRY(rp_n.alloc((size_t)n + 1));
    RWR_TRY(d_srcs.alloc(nb));
    RWR_TRY(d_cum.alloc(nb));
    if (links) {
        RWR_TRY(dst_n.alloc((size_t)m_new));
        RWR_TRY(et_n.alloc((size_t)m_new));
        RWR_TRY(w_n.alloc((size_t)m_new));
        RWR_TRY(wn_n.alloc((size_t)m_new));
        RWR_TRY(d_brk.alloc(nb));
        RWR_TRY(d_pos.alloc((size_t)count));
        RWR_TRY(d_dst.alloc((size_t)count));
        RWR_TRY(d_et.alloc((size_t)count));
        RWR_TRY(d_w.alloc((size_t)count));
    }
    // ... and of a call that adds nodes: the node SoA, the two ITEM orders, and every n-sized array the re-derive writes
    // (it fills them whole, as the first build does with its own fresh allocations)
    DevBuf<int64_t> nid_n, inp_n;
    DevBuf<uint8_t> nty_n, dang_n;
    DevBuf<double> wsrc_n;
    DevBuf<int32_t> ro_n, rox_n, irows_n, iord_n, d_bsorted;
    if (grow) {
        RWR_TRY(nid_n.alloc((size_t)n));
        RWR_TRY(nty_n.alloc((size_t)n));
        RWR_TRY(dang_n.alloc((size_t)n));
        RWR_TRY(wsrc_n.alloc((size_t)n));
        RWR_TRY(inp_n.alloc((size_t)n + 1));
        RWR_TRY(ro_n.alloc((size_t)n));
        RWR_TRY(rox_n.alloc((size_t)n));
        if (ni_new > 0) {
            RWR_TRY(irows_n.alloc((size_t)ni));
            RWR_TRY(iord_n.alloc((size_t)ni));
            RWR_TRY(d_bsorted.alloc((size_t)ni_new));
        }
    }
    AT("allocate new buffers");
    // the id range of the grown ITEM set (rwr_graph_create's sort-key parameters): the handle knows the largest resident id;
    // the smallest one is the last entry of the resident order, read back once per handle
    uint64_t key_lo = g->id_key_lo, key_hi = g->id_key_top;
    bool lo_known = g->id_key_lo_known != 0;
    if (grow && ni_new > 0 && ni_old > 0 && !lo_known) {
        int32_t last_row = 0;
        int64_t last_id = 0;
        RWR_HIP(hipMemcpy(&last_row, g->item_order.p + (ni_old - 1), sizeof(int32_t), hipMemcpyDeviceToHost));
        if (last_row < 0 || last_row >= n_old) { set_error("%s: the resident ITEM order is damaged", who); return RWR_E_HIP; }
        RWR_HIP(hipMemcpy(&last_id, g->node_id.p + last_row, sizeof(int64_t), hipMemcpyDeviceToHost));
        key_lo = nap_orderable(last_id);
        lo_known = true;
        AT("read back the smallest id");
    }
    if (ni_new > 0) {
        if (ni_old > 0) {
            key_lo = np.key_lo < key_lo ? np.key_lo : key_lo;
            key_hi = np.key_hi > key_hi ? np.key_hi : key_hi;
        } else {
            key_lo = np.key_lo;
            key_hi = np.key_hi;
            lo_known = true;
        }
    }
    // (a failure from here to the swap waits for the stream before it returns: the copies read this function's vectors and the
    //  kernels write its buffers, all of which go away on return -- and the handle, untouched, stays usable)
    auto merge = [&]() -> int32_t {
        if (nb > 0) {
            RWR_HIP(hipMemcpyAsync(d_srcs.p, plan.srcs.data(), sizeof(int32_t) * nb, hipMemcpyHostToDevice, s));
            RWR_HIP(hipMemcpyAsync(d_cum.p, plan.cum.data(), sizeof(int64_t) * nb, hipMemcpyHostToDevice, s));
        }
        if (links) {
            RWR_HIP(hipMemcpyAsync(d_brk.p, plan.brk.data(), sizeof(int64_t) * nb, hipMemcpyHostToDevice, s));
            RWR_HIP(hipMemcpyAsync(d_pos.p, plan.pos.data(), sizeof(int64_t) * (size_t)count, hipMemcpyHostToDevice, s));
            RWR_HIP(hipMemcpyAsync(d_dst.p, h_dst.data(), sizeof(int32_t) * (size_t)count, hipMemcpyHostToDevice, s));
            RWR_HIP(hipMemcpyAsync(d_et.p, h_et.data(), (size_t)count, hipMemcpyHostToDevice, s));
            RWR_HIP(hipMemcpyAsync(d_w.p, h_w.data(), sizeof(double) * (size_t)count, hipMemcpyHostToDevice, s));
        }
        hipLaunchKernelGGL(k_append_rowptr, dim3(cdiv((size_t)n + 1, 256)), dim3(256), 0, s, n, n_old, (int32_t)nb, d_srcs.p,
                           d_cum.p, g->rowptr.p, rp_n.p);
        if (links) {
            if (m_old > 0)
                hipLaunchKernelGGL(k_append_merge, dim3(cdiv((size_t)m_old, (size_t)AP_CHUNK)), dim3(AP_THREADS), 0, s, m_old,
                                   (int32_t)nb, d_brk.p, d_cum.p, g->dst.p, g->etype.p, g->w_raw.p, dst_n.p, et_n.p, w_n.p);
            hipLaunchKernelGGL(k_append_scatter, dim3(cdiv((size_t)count, 256)), dim3(256), 0, s, count, d_pos.p, d_dst.p,
                               d_et.p, d_w.p, dst_n.p, et_n.p, w_n.p);
        }
        if (grow) {
            // node SoA: the resident part device to device, the new tail from the caller's arrays
            RWR_HIP(hipMemcpyAsync(nid_n.p, g->node_id.p, sizeof(int64_t) * (size_t)n_old, hipMemcpyDeviceToDevice, s));
            RWR_HIP(hipMemcpyAsync(nid_n.p + n_old, node_id, sizeof(int64_t) * (size_t)n_new, hipMemcpyHostToDevice, s));
            RWR_HIP(hipMemcpyAsync(nty_n.p, g->node_type.p, (size_t)n_old, hipMemcpyDeviceToDevice, s));
            RWR_HIP(hipMemcpyAsync(nty_n.p + n_old, node_type, (size_t)n_new, hipMemcpyHostToDevice, s));
            if (ni_new > 0) {
                if (ni_old > 0)
                    RWR_HIP(hipMemcpyAsync(irows_n.p, g->item_rows.p, sizeof(int32_t) * (size_t)ni_old, hipMemcpyDeviceToDevice, s));
                RWR_HIP(hipMemcpyAsync(irows_n.p + ni_old, np.new_item_rows.data(), sizeof(int32_t) * (size_t)ni_new,
                                       hipMemcpyHostToDevice, s));
                RWR_HIP(hipMemcpyAsync(d_bsorted.p, np.new_item_sorted.data(), sizeof(int32_t) * (size_t)ni_new,
                                       hipMemcpyHostToDevice, s));
                hipLaunchKernelGGL(k_item_order_merge, dim3(cdiv((size_t)ni, 256)), dim3(256), 0, s, ni_old, ni_new,
                                   g->item_order.p, d_bsorted.p, nid_n.p, iord_n.p);
            }
        }
        RWR_HIP(hipGetLastError());
        RWR_HIP(hipStreamSynchronize(s));
        return RWR_OK;
    };
    RWR_TRY(idle_on_error(s, merge));
    AT("upload + merge kernels");
    // ---- phase 2: the handle takes the merged lists and the grown node arrays
    *swapped = true;
    growth.keep = true;
    swap_blocks(g->rowptr, rp_n);
    if (links) {
        swap_blocks(g->dst, dst_n);
        swap_blocks(g->etype, et_n);
        swap_blocks(g->w_raw, w_n);
        swap_blocks(g->w_norm_raw, wn_n);
    }
    node_append_shift_rowptr(g->h_rowptr, n, plan.srcs, plan.cum);
    g->nnz_raw = m_new;
    g->stats.nnz_raw = m_new;
    if (m_new > ONE_LAUNCH_MAX_M) g->staged = 0;                // past the one-launch build: the general derive from now on
    if (grow) {
        swap_blocks(g->node_id, nid_n);
        swap_blocks(g->node_type, nty_n);
        swap_blocks(g->dangling, dang_n);
        swap_blocks(g->w_src, wsrc_n);
        swap_blocks(g->in_ptr, inp_n);
        swap_blocks(g->row_order, ro_n);
        swap_blocks(g->row_order_x, rox_n);
        if (ni_new > 0) {
            swap_blocks(g->item_rows, irows_n);
            swap_blocks(g->item_order, iord_n);
            node_append_id_keys(true, key_lo, key_hi, &g->id_key_top, &g->id_key_bits);
            g->id_key_lo = key_lo;
            g->id_key_lo_known = lo_known ? 1 : 0;
        }
        g->h_is_item.resize((size_t)n, 0);                      // (reserved above)
        for (int32_t r : np.new_item_rows) g->h_is_item[(size_t)r] = 1;
        g->n = n;
        g->n_items = ni;
        g->stats.n = n;
        // a staged graph's pinned read-back area is sized for ONE_LAUNCH_MAX_N nodes (stage_layout.h: STAGE_BYTES)
        if (n > ONE_LAUNCH_MAX_N) g->staged = 0;
        // nothing cached for the old node count survives: the list a single-seed call left in pinned memory, and a
        // row-partitioned run (the re-derive ends it; its slab and seeds go too, so that only rwr_part_begin restarts it)
        g->sm_pin_count = -1;
        g->part_lo = g->part_hi = g->part_K = g->part_steps = 0;
        g->part_seeds.clear();
    }
    if (new_index_out && links) memcpy(new_index_out, plan.new_index.data(), sizeof(int64_t) * (size_t)count);
    AT("swap + host row pointers");
    const int32_t rc = graph_update_links(g, 0, nullptr, nullptr, nullptr);   // (count 0: the re-derive alone, build.hip)
    AT("re-derive");
    return rc;
}

}  // namespace rwr
