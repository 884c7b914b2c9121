// rwr_graph_append_links / rwr_graph_append_nodes: links appended to the lists of a resident graph, and
// nodes appended behind its last one.  The host plans (append_plan.h, node_append_plan.h) say where everything goes; the kernels
// here merge the resident raw lists with the new links, and the resident ITEM order with the new ITEM rows, into NEW buffers, the
// handle takes them, and build.hip's re-derive (the incremental rebuild with nothing to patch) rebuilds the walk's data from
// them -- the same kernels in the same order as rwr_graph_create, hence the same bits.
#include "edit.h"
#include "append_plan.h"
#include "node_append_plan.h"
#include "seg_copy.h"

#include <cstring>
#include <vector>

namespace rwr {

// ---- rwr_graph_append_links: the resident raw lists merged with a few new links, on the device.
// The host plan (append_plan.h) leaves one table entry per DISTINCT appended source s_j: brk[j] = rowptr_old[s_j + 1] and
// cum[j] = links appended to s_0 .. s_j.  The old flat position e moves to e + cum[upper_bound(brk, e) - 1]: between two
// breakpoints the move is constant, so the copy is a sequence of plain shifted block copies.
constexpr int AP_THREADS = SEG_THREADS;   // (seg_copy.h: the lanes of a segment's block copies)

static const Stamps append_stamps("append", "RWR_APPEND_TIMING");   // (engine.h; tools/append_latency.py)

// the new row pointers, i in [0, n]: one bisection over the distinct sources per row pointer (append_plan.h)
__global__ __launch_bounds__(256) void k_append_rowptr(int32_t n, int32_t n_old, int32_t nb, const int32_t *__restrict__ srcs,
                                                       const int64_t *__restrict__ cum, const int64_t *__restrict__ rp_old,
                                                       int64_t *__restrict__ rp_new)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    rp_new[i] = ap_rowptr_new(srcs, cum, nb, rp_old, n_old, i);
}

// A workgroup takes AP_CHUNK consecutive old positions and finds the breakpoints inside its chunk ONCE, brk[j .. jend) (every
// lane runs the same two bisections: uniform loads).  Then one of two paths, chosen per chunk:
// * sparse, at most AP_DENSE_BREAKS breakpoints in the chunk: it walks them, and each segment in between is three shifted
//   block copies without any search per element;
// * dense, more than that (a bulk append that touches most rows: segments of a few dozen elements, which would leave most
//   lanes idle in the block copies): every lane takes elements in lane order and finds each one's shift by bisecting the
//   chunk's OWN breakpoints -- at most 13 steps over entries the whole workgroup reads.  Loads stay lane-consecutive; the
//   stores of a wave fall into a few pieces of consecutive addresses.
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
    const ApSlice s = ap_chunk_slice(brk, nb, c0, c1);
    if (ap_chunk_dense(s)) {
        for (int64_t e = c0 + tid; e < c1; e += AP_THREADS) {
            const int64_t to = ap_dense_dest(brk, cum, s, e);
            w_n[to] = w_o[e];
            dst_n[to] = dst_o[e];
            et_n[to] = et_o[e];
        }
        return;
    }
    int j = s.j;
    for (int64_t a = c0; a < c1;) {
        const ApSeg g = ap_segment(brk, cum, nb, c1, a, j);
        copy_seg<double>(w_o, w_n, g.a, g.b, g.sh, tid);
        copy_seg<int32_t>(dst_o, dst_n, g.a, g.b, g.sh, tid);
        copy_seg_bytes(et_o, et_n, g.a, g.b, g.sh, tid);
        a = g.b;
        j = g.next;
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
    Stamps stamp = append_stamps.begin();
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
    stamp("plan (host)");
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
    stamp("new links in order (host)");
    // ---- phase 1: every buffer exists before anything is launched
    DevBuf<int64_t> rp_n, d_brk, d_cum, d_pos;
    DevBuf<int32_t> d_srcs, d_dst;
    DevBuf<uint8_t> d_et;
    DevBuf<double> d_w;
    StagedLinks ln;
    RWR_TRY(rp_n.alloc((size_t)n + 1));
    RWR_TRY(d_srcs.alloc(nb));
    RWR_TRY(d_cum.alloc(nb));
    if (links) {
        RWR_TRY(ln.alloc((size_t)m_new));
        RWR_TRY(d_brk.alloc(nb));
        RWR_TRY(d_pos.alloc((size_t)count));
        RWR_TRY(d_dst.alloc((size_t)count));
        RWR_TRY(d_et.alloc((size_t)count));
        RWR_TRY(d_w.alloc((size_t)count));
    }
    // ... and of a call that adds nodes: the node-sized arrays, with the two ITEM orders if an ITEM is among the new nodes
    StagedNodes nd;
    DevBuf<int32_t> d_bsorted;
    if (grow) {
        RWR_TRY(nd.alloc((size_t)n, (size_t)ni, ni_new > 0));
        if (ni_new > 0) RWR_TRY(d_bsorted.alloc((size_t)ni_new));
    }
    stamp("allocate new buffers");
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
        stamp("read back the smallest id");
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
                                   (int32_t)nb, d_brk.p, d_cum.p, g->dst.p, g->etype.p, g->w_raw.p, ln.dst.p, ln.etype.p, ln.w_raw.p);
            hipLaunchKernelGGL(k_append_scatter, dim3(cdiv((size_t)count, 256)), dim3(256), 0, s, count, d_pos.p, d_dst.p,
                               d_et.p, d_w.p, ln.dst.p, ln.etype.p, ln.w_raw.p);
        }
        if (grow) {
            // node SoA: the resident part device to device, the new tail from the caller's arrays
            RWR_HIP(hipMemcpyAsync(nd.node_id.p, g->node_id.p, sizeof(int64_t) * (size_t)n_old, hipMemcpyDeviceToDevice, s));
            RWR_HIP(hipMemcpyAsync(nd.node_id.p + n_old, node_id, sizeof(int64_t) * (size_t)n_new, hipMemcpyHostToDevice, s));
            RWR_HIP(hipMemcpyAsync(nd.node_type.p, g->node_type.p, (size_t)n_old, hipMemcpyDeviceToDevice, s));
            RWR_HIP(hipMemcpyAsync(nd.node_type.p + n_old, node_type, (size_t)n_new, hipMemcpyHostToDevice, s));
            if (ni_new > 0) {
                if (ni_old > 0)
                    RWR_HIP(hipMemcpyAsync(nd.item_rows.p, g->item_rows.p, sizeof(int32_t) * (size_t)ni_old, hipMemcpyDeviceToDevice, s));
                RWR_HIP(hipMemcpyAsync(nd.item_rows.p + ni_old, np.new_item_rows.data(), sizeof(int32_t) * (size_t)ni_new,
                                       hipMemcpyHostToDevice, s));
                RWR_HIP(hipMemcpyAsync(d_bsorted.p, np.new_item_sorted.data(), sizeof(int32_t) * (size_t)ni_new,
                                       hipMemcpyHostToDevice, s));
                hipLaunchKernelGGL(k_item_order_merge, dim3(cdiv((size_t)ni, 256)), dim3(256), 0, s, ni_old, ni_new,
                                   g->item_order.p, d_bsorted.p, nd.node_id.p, nd.item_order.p);
            }
        }
        RWR_HIP(hipGetLastError());
        RWR_HIP(hipStreamSynchronize(s));
        return RWR_OK;
    };
    RWR_TRY(idle_on_error(s, merge));
    stamp("upload + merge kernels");
    // ---- phase 2: the handle takes the merged lists and the grown node arrays
    *swapped = true;
    growth.keep = true;
    swap_blocks(g->rowptr, rp_n);
    if (links) ln.take(g);
    node_append_shift_rowptr(g->h_rowptr, n, plan.srcs, plan.cum);
    g->nnz_raw = m_new;
    g->stats.nnz_raw = m_new;
    if (m_new > ONE_LAUNCH_MAX_M) g->staged = 0;                // past the one-launch build: the general derive from now on
    if (grow) {
        nd.take(g);
        if (ni_new > 0) {
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
        forget_node_set(g, /*cand_lists=*/false);               // (the candidate lists stay: nodes were only appended)
    }
    if (new_index_out && links) memcpy(new_index_out, plan.new_index.data(), sizeof(int64_t) * (size_t)count);
    stamp("swap + host row pointers");
    const int32_t rc = graph_update_links(g, 0, nullptr, nullptr, nullptr);   // (count 0: the re-derive alone, build.hip)
    stamp("re-derive");
    return rc;
}

}  // namespace rwr
