// rwr_graph_remove_links: links leave the lists of a resident graph.  The host plan (remove_plan.h) sorts the
// removed positions; the kernels here compact the resident raw lists around them into NEW buffers, the handle takes them, and
// build.hip's re-derive (the incremental rebuild with nothing to patch) rebuilds the walk's data from them -- the same kernels
// in the same order as rwr_graph_create, hence the same bits.  The mirror image of append.hip's merge.
#include "edit.h"
#include "remove_plan.h"
#include "seg_copy.h"

#include <vector>

namespace rwr {

constexpr int RM_THREADS = SEG_THREADS;

static const Stamps remove_stamps("remove", "RWR_REMOVE_TIMING");   // (engine.h; tools/remove_latency.py)

// rowptr_new[i] = rowptr_old[i] - (removed positions in front of it), i in [0, n]: one bisection over r per row pointer
__global__ __launch_bounds__(256) void k_remove_rowptr(int32_t n, int64_t nr, const int64_t *__restrict__ r,
                                                       const int64_t *__restrict__ rp_old, int64_t *__restrict__ rp_new)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    rp_new[i] = rm_rowptr_new(r, nr, rp_old[i]);
}

// A workgroup takes RM_CHUNK consecutive old positions and finds the removed positions inside its chunk ONCE, r[j .. jend)
// (every lane runs the same two bisections: uniform loads).  Then one of two paths, chosen per chunk:
// * sparse, at most RM_DENSE_REMOVED of them: it walks the segments in between, and each one is three block copies shifted
//   down by a constant, without any search per element;
// * dense, more than that: every lane takes elements in lane order, bisects the chunk's own slice, skips the element if it is
//   a removed position and otherwise stores it at e - (removed positions in front of it).
// Both write every SURVIVING old position of the chunk exactly once, at e - shift(e), and read no removed one: the choice
// changes the speed, never the result.  e - shift(e) is strictly increasing over the survivors of the whole list
// (remove_plan.h), so it is one-to-one onto [0, m_new): the images of two chunks never overlap, every new position is written
// by exactly one workgroup, and the dword stores of the type array cover only bytes of the segment that issues them.
__global__ __launch_bounds__(RM_THREADS) void k_remove_compact(int64_t m_old, int64_t nr, const int64_t *__restrict__ r,
                                                               const int32_t *__restrict__ dst_o, const uint8_t *__restrict__ et_o,
                                                               const double *__restrict__ w_o, int32_t *__restrict__ dst_n,
                                                               uint8_t *__restrict__ et_n, double *__restrict__ w_n)
{
    const int tid = threadIdx.x;
    const int64_t c0 = (int64_t)blockIdx.x * RM_CHUNK;
    const int64_t c1 = c0 + RM_CHUNK < m_old ? c0 + RM_CHUNK : m_old;
    const RmSlice s = rm_chunk_slice(r, nr, c0, c1);
    if (rm_chunk_dense(s)) {
        // (at most 13 steps over entries the whole workgroup reads; loads stay lane-consecutive, and the stores of a wave fall
        //  into a few pieces of consecutive addresses)
        for (int64_t e = c0 + tid; e < c1; e += RM_THREADS) {
            int64_t to;
            if (!rm_dense_dest(r, s, e, &to)) continue;
            w_n[to] = w_o[e];
            dst_n[to] = dst_o[e];
            et_n[to] = et_o[e];
        }
        return;
    }
    for (int64_t t = 0; t <= s.jend - s.j; ++t) {
        const RmSeg g = rm_segment(r, s, c0, c1, t);
        if (g.b <= g.a) continue;                               // (neighbouring removed positions)
        copy_seg<double>(w_o, w_n, g.a, g.b, -g.sh, tid);
        copy_seg<int32_t>(dst_o, dst_n, g.a, g.b, -g.sh, tid);
        copy_seg_bytes(et_o, et_n, g.a, g.b, -g.sh, tid);
    }
}

// Removes the links at link_index[0 .. count) from the resident raw lists and re-derives.  Two phases, as graph_append:
// everything up to the swap works on NEW buffers -- an argument error or a failed allocation leaves the graph as it was --
// and from the swap on (*swapped) a failure leaves raw and derived arrays out of step, as in graph_update_links.
int32_t graph_remove(rwr_graph *g, int64_t count, const int64_t *link_index, bool *swapped)
{
    const int32_t n = g->n;
    hipStream_t s = g->stream;
    *swapped = false;
    Stamps stamp = remove_stamps.begin();
    RemovePlan plan = remove_plan(n, g->h_rowptr.data(), count, link_index);
    if (plan.verdict == REMOVE_BAD_RANGE) {
        set_error("rwr_graph_remove_links: link_index[%lld] = %lld is outside [0, %lld)", (long long)plan.bad_q,
                  (long long)link_index[plan.bad_q], (long long)plan.m_old);
        return RWR_E_RANGE;
    }
    if (plan.verdict == REMOVE_DUPLICATE) {
        set_error("rwr_graph_remove_links: link_index[%lld] = %lld was given before: every position at most once",
                  (long long)plan.bad_q, (long long)link_index[plan.bad_q]);
        return RWR_E_INVALID;
    }
    if (count <= 0) {
        *swapped = true;               // (nothing to compact: a plain rebuild, with rwr_graph_update_links' failure rule)
        return graph_update_links(g, 0, nullptr, nullptr, nullptr);
    }
    const int64_t m_old = plan.m_old, m_new = plan.m_new;       // (count > 0 passed the range check: m_old > 0)
    stamp("plan (host)");
    // ---- phase 1: every buffer exists before anything is launched (a length of 0 is a block of one element, as in the build)
    DevBuf<int64_t> rp_n, d_r;
    StagedLinks ln;
    RWR_TRY(rp_n.alloc((size_t)n + 1));
    RWR_TRY(d_r.alloc((size_t)count));
    RWR_TRY(ln.alloc((size_t)m_new));
    stamp("allocate new buffers");
    // (a failure from here to the swap waits for the stream before it returns: the copy reads the plan's vector and the kernels
    //  write this function's buffers, all of which go away on return -- and the handle, untouched, stays usable)
    auto compact = [&]() -> int32_t {
        RWR_HIP(hipMemcpyAsync(d_r.p, plan.r.data(), sizeof(int64_t) * (size_t)count, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_remove_rowptr, dim3(cdiv((size_t)n + 1, 256)), dim3(256), 0, s, n, count, d_r.p, g->rowptr.p, rp_n.p);
        hipLaunchKernelGGL(k_remove_compact, dim3(cdiv((size_t)m_old, (size_t)RM_CHUNK)), dim3(RM_THREADS), 0, s, m_old, count,
                           d_r.p, g->dst.p, g->etype.p, g->w_raw.p, ln.dst.p, ln.etype.p, ln.w_raw.p);
        RWR_HIP(hipGetLastError());
        RWR_HIP(hipStreamSynchronize(s));
        return RWR_OK;
    };
    RWR_TRY(idle_on_error(s, compact));
    stamp("upload + compaction kernels");
    // ---- phase 2: the handle takes the shortened lists
    *swapped = true;
    swap_blocks(g->rowptr, rp_n);
    ln.take(g);
    g->h_rowptr.swap(plan.rowptr_new);
    g->nnz_raw = m_new;
    g->stats.nnz_raw = m_new;
    // (g->staged stays as it is: a handle that left the one-launch build does not go back when the link count drops below
    //  ONE_LAUNCH_MAX_M again; the general derive gives the same bits)
    stamp("swap + host row pointers");
    const int32_t rc = graph_update_links(g, 0, nullptr, nullptr, nullptr);   // (count 0: the re-derive alone, build.hip)
    stamp("re-derive");
    return rc;
}

}  // namespace rwr
