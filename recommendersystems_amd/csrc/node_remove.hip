// rwr_graph_remove_nodes: nodes leave a resident graph, with every link from or to them, and the others close
// up.  The host plan (node_remove_plan.h) validates the list and knows the removed ROWS; which links point TO a removed node
// only the resident dst array tells, so the kernels here count, scan and scatter the raw lists around both kinds into NEW
// buffers, renumber every surviving target, compact the node arrays and the two ITEM orders, and hand the new row pointers
// back.  The handle takes the buffers when all of it is done, and build.hip's re-derive (the incremental rebuild with nothing
// to patch) rebuilds the walk's data from them -- the same kernels in the same order as rwr_graph_create, hence the same bits.
#include "edit.h"
#include "filter.h"
#include "node_append_plan.h"
#include "node_remove_plan.h"

#include <cstring>
#include <vector>

namespace rwr {

static const Stamps node_remove_stamps("remove_nodes", "RWR_NODE_REMOVE_TIMING");   // (engine.h; tools/remove_nodes_latency.py)

// what every kernel over the links reads besides the links
struct NrmTables {
    int32_t n;                     // nodes before the call
    int64_t m_old, ni;             // links before the call, removed intervals
    const int64_t *iv_lo, *iv_hi;
    const uint8_t *bits;           // removed-node bitmap, (n + 7) / 8 bytes: L2-resident
};

// the chunk [c0, c1) of workgroup b (an empty one for a graph without links)
__device__ __forceinline__ void nrm_chunk(int64_t m_old, int64_t *c0, int64_t *c1)
{
    *c0 = (int64_t)blockIdx.x * NRM_CHUNK;
    *c1 = *c0 + NRM_CHUNK < m_old ? *c0 + NRM_CHUNK : m_old;
}

// 1. count: cnt[chunk] = kept links of the chunk.  dst is loaded lane-consecutively; the slice of the intervals is found once,
// by bisections every lane runs alike.
__global__ __launch_bounds__(NRM_THREADS) void k_nrm_count(NrmTables T, const int32_t *__restrict__ dst_o, int64_t *__restrict__ cnt)
{
    __shared__ int wc[NRM_WAVES];
    const int tid = threadIdx.x, lane = tid & (NRM_WAVE - 1), wv = tid / NRM_WAVE;
    int64_t c0, c1;
    nrm_chunk(T.m_old, &c0, &c1);
    const NrmSlice s = nrm_chunk_slice(T.iv_lo, T.iv_hi, T.ni, c0, c1);
    int mine = 0;                                                  // (the wave's count, in every lane)
    for (int64_t t0 = c0; t0 < c1; t0 += NRM_THREADS) {
        const int64_t e = t0 + tid;
        const bool k = e < c1 && nrm_keep(T.iv_lo, T.iv_hi, s, T.bits, T.n, e, dst_o[e]);
        mine += nrm_wave_count(__ballot(k));
    }
    if (lane == 0) wc[wv] = mine;
    __syncthreads();
    if (tid == 0) {
        int c = 0;
        for (int q = 0; q < NRM_WAVES; ++q) c += wc[q];
        cnt[blockIdx.x] = c;
    }
}

// 2. scan: the chunks' counts to exclusive offsets in place, off[nchunks] = their sum -- launch_cand_scan (typed.hip) in 64 bits.

// 3. scatter.  The workgroup recomputes the predicate trip by trip and ranks its kept links stably: the element of trip t, wave
// wv, lane l stands behind the kept elements of the earlier trips (base), of the lower waves of its trip (wc) and of the lower
// lanes of its wave (the ballot) -- nrm_rank_in_chunk.  A kept link goes to off[chunk] + rank with its target renumbered.  The
// rank of EVERY element of the chunk, kept or not, stays in LDS (pre: 8 193 x 2 bytes), because it is what a row pointer needs:
// a surviving row whose old start falls into this chunk starts at off[chunk] + pre[start - c0] in the new list.  The last
// chunk also takes the starts equal to m_old (trailing rows without links, and the end, "row" n with new index n_new).
// Every new link position, every new row pointer and every entry of link_out is written once, by one workgroup.
__global__ __launch_bounds__(NRM_THREADS) void k_nrm_scatter(NrmTables T, const int32_t *__restrict__ new_index,
                                                             const int64_t *__restrict__ rp_old, const int32_t *__restrict__ dst_o,
                                                             const uint8_t *__restrict__ et_o, const double *__restrict__ w_o,
                                                             const int64_t *__restrict__ off, int64_t m_cap,
                                                             int32_t *__restrict__ dst_n, uint8_t *__restrict__ et_n,
                                                             double *__restrict__ w_n, int64_t *__restrict__ rp_n,
                                                             int64_t *__restrict__ link_out)
{
    __shared__ uint16_t pre[NRM_CHUNK + 1];
    __shared__ int wc[2][NRM_WAVES];
    const int tid = threadIdx.x, lane = tid & (NRM_WAVE - 1), wv = tid / NRM_WAVE;
    int64_t c0, c1;
    nrm_chunk(T.m_old, &c0, &c1);
    const NrmSlice s = nrm_chunk_slice(T.iv_lo, T.iv_hi, T.ni, c0, c1);
    const int64_t o = off[blockIdx.x];
    int base = 0;
    int trip = 0;
    for (int64_t t0 = c0; t0 < c1; t0 += NRM_THREADS, ++trip) {
        const int64_t e = t0 + tid;
        const bool in = e < c1;
        const int32_t d = in ? dst_o[e] : 0;
        const bool k = in && nrm_keep(T.iv_lo, T.iv_hi, s, T.bits, T.n, e, d);
        const unsigned long long bal = __ballot(k);
        int *w2 = wc[trip & 1];            // (two sets: the next trip's counts are written while a slow wave still reads these)
        if (lane == 0) w2[wv] = nrm_wave_count(bal);
        __syncthreads();
        const int rank = nrm_rank_in_chunk(base, w2, wv, bal, lane);
        if (in) {
            pre[e - c0] = (uint16_t)rank;
            const int64_t to = o + rank;
            if (k && to < m_cap) {         // (to < m_new <= m_cap by construction)
                w_n[to] = w_o[e];
                dst_n[to] = new_index[d];
                et_n[to] = et_o[e];
            }
            if (link_out) link_out[e] = k ? to : (int64_t)-1;
        }
        for (int q = 0; q < NRM_WAVES; ++q) base += w2[q];
    }
    const bool last = blockIdx.x + 1 == gridDim.x;
    if (tid == 0) pre[c1 - c0] = (uint16_t)base;                     // (the chunk's count: at most 8 192)
    __syncthreads();
    const NrmRows rows = nrm_chunk_rows(rp_old, T.n, c0, c1, last);
    for (int64_t i = rows.lo + tid; i < rows.hi; i += NRM_THREADS) {
        const int32_t to = new_index[i];
        if (to >= 0) rp_n[to] = o + pre[rp_old[i] - c0];
    }
}

// 4. node arrays: one thread per old node
__global__ __launch_bounds__(256) void k_nrm_nodes(int32_t n, const int32_t *__restrict__ new_index, const int64_t *__restrict__ id_o,
                                                   const uint8_t *__restrict__ ty_o, int64_t *__restrict__ id_n,
                                                   uint8_t *__restrict__ ty_n)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t to = new_index[i];
    if (to < 0) return;
    id_n[to] = id_o[i];
    ty_n[to] = ty_o[i];
}

// 5. / 6. a list of rows (item_rows: ascending; item_order: ids descending, equal ids row-ascending) without the removed rows,
// the others renumbered, in the list's order: count per block of NRM_THREADS entries, launch_cand_scan, ordered scatter -- the
// compaction of typed.hip's candidate lists with the bitmap as its match.  new_index is monotone over the survivors, so an
// ascending list stays ascending and equal ids stay row-ascending.
__device__ __forceinline__ bool nrm_list_match(int32_t n, int32_t len, const int32_t *__restrict__ list, const uint8_t *__restrict__ bits,
                                               int *wc, unsigned long long *bal, int32_t *row)
{
    const int64_t q = (int64_t)blockIdx.x * NRM_THREADS + threadIdx.x;
    *row = q < len ? list[q] : -1;
    const bool m = (uint32_t)*row < (uint32_t)n && !nrm_removed(bits, *row);
    *bal = __ballot(m);
    if ((threadIdx.x & (NRM_WAVE - 1)) == 0) wc[threadIdx.x / NRM_WAVE] = nrm_wave_count(*bal);
    __syncthreads();
    return m;
}
__global__ __launch_bounds__(NRM_THREADS) void k_nrm_list_count(int32_t n, int32_t len, const int32_t *__restrict__ list,
                                                                const uint8_t *__restrict__ bits, int32_t *__restrict__ cnt)
{
    __shared__ int wc[NRM_WAVES];
    unsigned long long bal;
    int32_t row;
    nrm_list_match(n, len, list, bits, wc, &bal, &row);
    if (threadIdx.x == 0) {
        int c = 0;
        for (int q = 0; q < NRM_WAVES; ++q) c += wc[q];
        cnt[blockIdx.x] = c;
    }
}
__global__ __launch_bounds__(NRM_THREADS) void k_nrm_list_scatter(int32_t n, int32_t len, const int32_t *__restrict__ list,
                                                                  const uint8_t *__restrict__ bits, const int32_t *__restrict__ new_index,
                                                                  const int32_t *__restrict__ off, int32_t total, int32_t *__restrict__ out)
{
    __shared__ int wc[NRM_WAVES];
    unsigned long long bal;
    int32_t row;
    if (!nrm_list_match(n, len, list, bits, wc, &bal, &row)) return;
    const int pos = off[blockIdx.x] + nrm_rank_in_chunk(0, wc, threadIdx.x / NRM_WAVE, bal, threadIdx.x & (NRM_WAVE - 1));
    if (pos >= 0 && pos < total) out[pos] = new_index[row];
}

// 7. the ids of the first and the last entry of the new item_order: the largest and the smallest surviving ITEM id
__global__ void k_nrm_id_ends(int32_t n_new, int32_t ni_new, const int32_t *__restrict__ iord_n, const int64_t *__restrict__ id_n,
                              int64_t *__restrict__ ends)
{
    if (threadIdx.x > 1 || blockIdx.x > 0) return;
    const int32_t row = iord_n[threadIdx.x == 0 ? 0 : ni_new - 1];
    ends[threadIdx.x] = (uint32_t)row < (uint32_t)n_new ? id_n[row] : 0;
}

// Removes the nodes node_index[0 .. count) with their links from the resident graph and re-derives.  Two phases, as
// graph_append: everything up to the swap works on NEW buffers -- an argument error or a failed allocation leaves the graph as
// it was -- and from the swap on (*swapped) a failure leaves raw and derived arrays out of step, as in graph_update_links.
// The outputs are written last, when nothing can fail any more.
int32_t graph_remove_nodes(rwr_graph *g, int32_t count, const int32_t *node_index, int32_t *new_node_index_out,
                           int64_t *new_link_index_out, int64_t *links_removed_out, bool *swapped)
{
    const int32_t n = g->n;
    hipStream_t s = g->stream;
    *swapped = false;
    Stamps stamp = node_remove_stamps.begin();
    NodeRemovePlan plan = node_remove_plan(n, g->h_rowptr.data(), g->h_is_item.data(), count, node_index);
    if (plan.verdict == NODE_REMOVE_BAD_RANGE) {
        set_error("rwr_graph_remove_nodes: node_index[%d] = %d is outside [0, %d)", plan.bad_q, node_index[plan.bad_q], n);
        return RWR_E_RANGE;
    }
    if (plan.verdict == NODE_REMOVE_DUPLICATE) {
        set_error("rwr_graph_remove_nodes: node_index[%d] = %d was given before: every node at most once", plan.bad_q,
                  node_index[plan.bad_q]);
        return RWR_E_INVALID;
    }
    if (plan.verdict == NODE_REMOVE_ALL) {
        set_error("rwr_graph_remove_nodes: all %d nodes would leave and a graph has at least one: destroy the graph instead", n);
        return RWR_E_UNSUPPORTED;
    }
    const int64_t m_old = plan.m_old;
    if (count <= 0) {
        *swapped = true;               // (nothing to compact: a plain rebuild, with rwr_graph_update_links' failure rule)
        RWR_TRY(graph_update_links(g, 0, nullptr, nullptr, nullptr));
        if (new_node_index_out)
            for (int32_t i = 0; i < n; ++i) new_node_index_out[i] = i;
        if (new_link_index_out)
            for (int64_t e = 0; e < m_old; ++e) new_link_index_out[e] = e;
        if (links_removed_out) *links_removed_out = 0;
        return RWR_OK;
    }
    const int32_t n_new = plan.n_new, ni_old = g->n_items, ni_new = plan.n_items_new;
    const int64_t m_cap = m_old - plan.m_rows;      // the new list is at most this long: the link buffers' size
    const int64_t nchunks = nrm_chunks(m_old), ni = (int64_t)plan.iv_lo.size();
    const int32_t lb = nrm_list_blocks(ni_old);
    std::vector<int64_t> h_rp_new((size_t)n_new + 1);
    stamp("plan (host)");
    // ---- phase 1: every buffer exists before anything is launched (a length of 0 is a block of one element, as in the build)
    DevBuf<int64_t> rp_n, d_ivlo, d_ivhi, d_off, d_ends, d_link;
    DevBuf<int32_t> d_newidx, d_loff;
    DevBuf<uint8_t> d_bits;
    StagedLinks ln;
    StagedNodes nd;
    RWR_TRY(rp_n.alloc((size_t)n_new + 1));
    RWR_TRY(d_ivlo.alloc((size_t)ni));
    RWR_TRY(d_ivhi.alloc((size_t)ni));
    RWR_TRY(d_off.alloc((size_t)nchunks + 1));
    RWR_TRY(d_bits.alloc(plan.bits.size()));
    RWR_TRY(d_newidx.alloc((size_t)n + 1));
    RWR_TRY(ln.alloc((size_t)m_cap));
    if (new_link_index_out) RWR_TRY(d_link.alloc((size_t)m_old));
    // ... the node-sized arrays and the two ITEM orders (§3.13's table)
    RWR_TRY(nd.alloc((size_t)n_new, (size_t)ni_new, /*with_item_lists=*/true));
    RWR_TRY(d_loff.alloc((size_t)lb + 1));
    RWR_TRY(d_ends.alloc(2));
    stamp("allocate new buffers");
    int64_t h_ends[2] = {0, 0};
    // (a failure from here to the swap waits for the stream before it returns: the copies read the plan's vectors and the kernels
    //  write this function's buffers, all of which go away on return -- and the handle, untouched, stays usable)
    auto compact = [&]() -> int32_t {
        RWR_HIP(hipMemcpyAsync(d_bits.p, plan.bits.data(), plan.bits.size(), hipMemcpyHostToDevice, s));
        RWR_HIP(hipMemcpyAsync(d_newidx.p, plan.new_index.data(), sizeof(int32_t) * ((size_t)n + 1), hipMemcpyHostToDevice, s));
        if (ni > 0) {
            RWR_HIP(hipMemcpyAsync(d_ivlo.p, plan.iv_lo.data(), sizeof(int64_t) * (size_t)ni, hipMemcpyHostToDevice, s));
            RWR_HIP(hipMemcpyAsync(d_ivhi.p, plan.iv_hi.data(), sizeof(int64_t) * (size_t)ni, hipMemcpyHostToDevice, s));
        }
        const NrmTables T{n, m_old, ni, d_ivlo.p, d_ivhi.p, d_bits.p};
        hipLaunchKernelGGL(k_nrm_count, dim3((unsigned)nchunks), dim3(NRM_THREADS), 0, s, T, g->dst.p, d_off.p);
        launch_cand_scan(nchunks, d_off.p, s);
        hipLaunchKernelGGL(k_nrm_scatter, dim3((unsigned)nchunks), dim3(NRM_THREADS), 0, s, T, d_newidx.p, g->rowptr.p, g->dst.p,
                           g->etype.p, g->w_raw.p, d_off.p, m_cap, ln.dst.p, ln.etype.p, ln.w_raw.p, rp_n.p,
                           new_link_index_out ? d_link.p : (int64_t *)nullptr);
        hipLaunchKernelGGL(k_nrm_nodes, dim3(cdiv((size_t)n, 256)), dim3(256), 0, s, n, d_newidx.p, g->node_id.p, g->node_type.p,
                           nd.node_id.p, nd.node_type.p);
        if (lb > 0) {
            const int32_t *lists[2] = {g->item_rows.p, g->item_order.p};
            int32_t *outs[2] = {nd.item_rows.p, nd.item_order.p};
            for (int a = 0; a < 2; ++a) {                            // (one offset table: the stream runs them in turn)
                hipLaunchKernelGGL(k_nrm_list_count, dim3((unsigned)lb), dim3(NRM_THREADS), 0, s, n, ni_old, lists[a], d_bits.p, d_loff.p);
                launch_cand_scan(lb, d_loff.p, s);
                hipLaunchKernelGGL(k_nrm_list_scatter, dim3((unsigned)lb), dim3(NRM_THREADS), 0, s, n, ni_old, lists[a], d_bits.p,
                                   d_newidx.p, d_loff.p, ni_new, outs[a]);
            }
        }
        if (ni_new > 0) {
            hipLaunchKernelGGL(k_nrm_id_ends, dim3(1), dim3(NRM_WAVE), 0, s, n_new, ni_new, nd.item_order.p, nd.node_id.p, d_ends.p);
            RWR_HIP(hipMemcpyAsync(h_ends, d_ends.p, sizeof(h_ends), hipMemcpyDeviceToHost, s));
        }
        RWR_HIP(hipGetLastError());
        // the one read-back of the call besides the optional outputs: the new row pointers
        RWR_HIP(hipMemcpyAsync(h_rp_new.data(), rp_n.p, sizeof(int64_t) * ((size_t)n_new + 1), hipMemcpyDeviceToHost, s));
        RWR_HIP(hipStreamSynchronize(s));
        return RWR_OK;
    };
    RWR_TRY(idle_on_error(s, compact));
    const int64_t m_new = h_rp_new[(size_t)n_new];
    if (h_rp_new[0] != 0 || m_new < 0 || m_new > m_cap) {
        set_error("rwr_graph_remove_nodes: the compaction left %lld links of at most %lld", (long long)m_new, (long long)m_cap);
        return RWR_E_HIP;
    }
    stamp("upload + compaction kernels");
    // ---- phase 2: the handle takes the shortened lists and the smaller node arrays
    *swapped = true;
    swap_blocks(g->rowptr, rp_n);
    ln.take(g);
    nd.take(g);
    g->h_rowptr.swap(h_rp_new);                                 // (exchanges: nothing on the host can fail here)
    g->h_is_item.swap(plan.is_item_new);
    g->n = n_new;
    g->n_items = ni_new;
    g->nnz_raw = m_new;
    g->stats.n = n_new;
    g->stats.nnz_raw = m_new;
    // rwr_graph_create's sort-key parameters for the surviving ITEM ids (no ITEM left: its values for n_items == 0)
    const uint64_t key_hi = ni_new > 0 ? nap_orderable(h_ends[0]) : 0, key_lo = ni_new > 0 ? nap_orderable(h_ends[1]) : 0;
    node_append_id_keys(ni_new > 0, key_lo, key_hi, &g->id_key_top, &g->id_key_bits);
    g->id_key_lo = key_lo;
    g->id_key_lo_known = 1;
    // (g->staged stays as it is: a staged handle stays staged, and one that left the one-launch build does not go back when n or
    //  the link count drop below its limits again; the general derive gives the same bits)
    forget_node_set(g, /*cand_lists=*/true);                    // (the one edit after which the same n can stand for other rows)
    stamp("swap + host state");
    const int32_t rc = graph_update_links(g, 0, nullptr, nullptr, nullptr);   // (count 0: the re-derive alone, build.hip)
    stamp("re-derive");
    if (rc != RWR_OK) return rc;
    if (new_link_index_out && m_old > 0)
        RWR_HIP(hipMemcpy(new_link_index_out, d_link.p, sizeof(int64_t) * (size_t)m_old, hipMemcpyDeviceToHost));
    if (new_node_index_out) memcpy(new_node_index_out, plan.new_index.data(), sizeof(int32_t) * (size_t)n);
    if (links_removed_out) *links_removed_out = m_old - m_new;
    stamp("outputs");
    return RWR_OK;
}

}  // namespace rwr
