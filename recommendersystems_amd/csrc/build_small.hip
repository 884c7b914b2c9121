// Host side of the one-launch build of ego-network-sized graphs (kernels: build.hip, k_build_small / k_build_small_multi): which
// graphs take it, the argument block and scratch of one graph, the read-back, and the two drivers -- graph_derive_small for one
// handle, graphs_build_multi for a batch of them.
#include "build.h"
#include "key_bits.h"

#include <vector>
#include <cstdlib>
#include <cstring>

namespace rwr {

// THE predicate of the staged upload and the one-launch build (the two knobs: experiments build only)
bool graph_fits_small_build(int32_t n, int64_t m)
{
    static const int stage_env = [] { const char *e = RWR_TUNE_ENV("RWR_STAGE"); return e ? atoi(e) : 1; }();
    return stage_env && row_order_mode() == 0 && n > 0 && n <= ONE_LAUNCH_MAX_N && m >= 0 && m <= ONE_LAUNCH_MAX_M;
}
// ... of a handle: uploaded through its staging buffer and (after appends) still inside the limits
bool small_build_ok(const rwr_graph *g) { return g->staged && g->sm_stage && graph_fits_small_build(g->n, g->nnz_raw); }

// ---- the build in two halves around its launch: a single graph launches k_build_small in between (graph_derive_small), a batch
// of graphs one k_build_small_multi for all of them (graphs_build_multi)
struct SmallBuild {
    DevBuf<int32_t> esrc;
    DevBuf<uint32_t> skey, skey2, sval, sval2, ival, ival2;
    DevBuf<uint64_t> ikey, ikey2;
    DevBuf<int> flags;
    BuildSmallArgs a{};
};
static int32_t small_build_begin(rwr_graph *g, bool first, SmallBuild &b)
{
    const int32_t n = g->n;
    const int64_t m = g->nnz_raw;
    // the (key, value) buffers serve the link sort (m entries) AND, afterwards, the row-order / item sorts (n entries)
    const size_t kv = (size_t)(m > (int64_t)n ? m : (int64_t)n);
    RWR_TRY(b.esrc.alloc(m));
    RWR_TRY(b.skey.alloc(kv));
    RWR_TRY(b.skey2.alloc(kv));
    RWR_TRY(b.sval.alloc(kv));
    RWR_TRY(b.sval2.alloc(kv));
    RWR_TRY(b.flags.alloc(4));
    RWR_TRY(b.ikey.alloc(n));
    RWR_TRY(b.ikey2.alloc(n));
    RWR_TRY(b.ival.alloc(n));
    RWR_TRY(b.ival2.alloc(n));
    RWR_TRY(g->in_src.ensure((size_t)m + 64));
    RWR_TRY(g->in_w.ensure((size_t)(m > 0 ? m : 1)));
    BuildSmallArgs &a = b.a;
    a = BuildSmallArgs{};
    a.n = n; a.n_items = g->n_items; a.first = first ? 1 : 0; a.do_stage_in = g->stage_pending ? 1 : 0; a.m = m;
    a.zero_flags = 1;
    a.stage = g->stage_dev_ext ? g->stage_dev_ext : g->d_stage.p; a.L = stage_layout(n, m);
    a.node_id = g->node_id.p; a.node_type = g->node_type.p; a.rowptr = g->rowptr.p; a.dst = g->dst.p; a.etype = g->etype.p;
    a.w_raw = g->w_raw.p; a.w_norm = g->w_norm_raw.p; a.esrc = b.esrc.p; a.skey = b.skey.p; a.skey2 = b.skey2.p; a.sval = b.sval.p;
    a.sval2 = b.sval2.p; a.dangling = g->dangling.p; a.w_src = g->w_src.p; a.flags = b.flags.p; a.in_ptr = g->in_ptr.p;
    a.in_src = g->in_src.p; a.in_w = g->in_w.p; a.row_order = g->row_order.p; a.row_order_x = g->row_order_x.p;
    a.item_rows = g->item_rows.p; a.item_order = g->item_order.p; a.ikey = b.ikey.p; a.ikey2 = b.ikey2.p; a.ival = b.ival.p;
    a.ival2 = b.ival2.p;
    a.order_mode = 0;
    a.n_bits = bit_length((uint64_t)n);
    a.id_key_top = g->id_key_top; a.id_key_bits = g->id_key_bits;
    a.pin_out = g->sm_out ? g->sm_out : static_cast<uint8_t *>(g->sm_stage) + STAGE_OUT_OFF;
    a.stamps = nullptr;
    return RWR_OK;
}
// after the stream the build ran on has been synchronised
static int32_t small_build_end(rwr_graph *g, SmallBuild &b, hipEvent_t e0, hipEvent_t e1)
{
    const int32_t n = g->n;
    const uint8_t *pin = b.a.pin_out;
    int h_flags[4];
    g->stage_pending = 0;
    g->h_in_ptr.resize((size_t)n + 1);
    g->h_dangling.resize((size_t)n);
    memcpy(h_flags, pin + STAGE_OUT_FLAGS, sizeof(h_flags));
    memcpy(g->h_in_ptr.data(), pin + STAGE_OUT_IN_PTR, sizeof(int64_t) * ((size_t)n + 1));
    memcpy(g->h_dangling.data(), pin + stage_out_dangling(n), (size_t)n);
    // (vf or not, in_w stays: small.hip reads it)
    RWR_TRY(graph_apply_flags(g, *reinterpret_cast<const int64_t *>(pin + STAGE_OUT_NNZ), h_flags));
    return derive_finish(g, h_flags, e0, e1);
}

int32_t graph_derive_small(rwr_graph *g, bool first)
{
    hipStream_t s = g->stream;
    Stamps stamp = build_stamps.begin();
    hipEvent_t e0 = g->ev_a, e1 = g->ev_b;
    SmallBuild b;
    RWR_TRY(small_build_begin(g, first, b));
    stamp("derive allocs");
#ifdef RWR_EXPERIMENTS
    DevBuf<unsigned long long> stamps_d;
    if (build_stamps.on()) { RWR_TRY(stamps_d.alloc(8)); b.a.stamps = stamps_d.p; }
#endif
    RWR_HIP(hipEventRecord(e0, s));
    RWR_TRY(launch_build_small(b.a, s));
    RWR_HIP(hipEventRecord(e1, s));
    stamp("enqueue one-launch build");
    RWR_HIP(hipStreamSynchronize(s));                      // the ONE synchronisation of an ego-network-sized build
    stamp("sync (whole build)");
#ifdef RWR_EXPERIMENTS
    if (build_stamps.on()) {
        unsigned long long hs[8];
        RWR_HIP(hipMemcpy(hs, stamps_d.p, sizeof(hs), hipMemcpyDeviceToHost));
        unsigned long long rp[16];
        row_pass_stamps(rp);
        fprintf(stderr, "[build] row pass of group 0 (us): setup %.1f sweep1 %.1f sweep2 %.1f; started %.1f after stage 1\n", (rp[1] - rp[0]) / 100.0,
                (rp[2] - rp[1]) / 100.0, (rp[3] - rp[2]) / 100.0, (rp[0] - hs[1]) / 100.0);
        fprintf(stderr, "[build] k_build_small stages (us): unpack %.1f rows %.1f linksort %.1f in_ptr+gather %.1f orders %.1f items %.1f out %.1f\n",
                (hs[1] - hs[0]) / 100.0, (hs[2] - hs[1]) / 100.0, (hs[3] - hs[2]) / 100.0, (hs[4] - hs[3]) / 100.0, (hs[5] - hs[4]) / 100.0,
                (hs[6] - hs[5]) / 100.0, (hs[7] - hs[6]) / 100.0);
    }
#endif
    return small_build_end(g, b, e0, e1);
}

// ---------------------------------------------------------------------------------------------------------------------
// A batch of ego-network-sized graphs built with ONE launch (rwr_eval_graphs, eval_graphs.hip: graphs_build_multi here, then
// recommend_small_multi in small.hip and eval_ranked_multi in rank.hip).  The reference builds one such
// graph per fold and methodology (Experiment.cs:69-105) and ten of its threads do so at once (Program.cs:11); handled one
// graph per call that is two synchronisations and a dozen runtime calls per graph, and the threads queue up behind the
// runtime rather than the GPU.  Here every graph of the batch gets a workgroup of k_build_small_multi: one H2D copy of all
// staging slots, one launch, one synchronisation.  The arena is slot 0 of the thread's pinned buffers (pool.hip: multi_pinned).
//   caller_index[i]: the graph's number in the caller's batch (for error messages).
int32_t graphs_build_multi(rwr_graph **gs, int32_t count, const rwr_graph_desc *descs, const int32_t *caller_index, hipStream_t s)
{
    if (count <= 0) return RWR_OK;
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    // arena: [staging slots of all graphs, contiguous][read-back areas]
    std::vector<size_t> in_off((size_t)count + 1, 0), out_off((size_t)count + 1, 0);
    for (int32_t i = 0; i < count; ++i) {
        const int32_t n = descs[i].n_nodes;
        const int64_t m = descs[i].rowptr[n];
        in_off[(size_t)i + 1] = in_off[i] + up(stage_layout(n, m).total + 8);
        out_off[(size_t)i + 1] = out_off[i] + up(stage_out_bytes(n));
    }
    const size_t in_bytes = in_off[count], need = in_bytes + out_off[count];
    void *pin_v = nullptr, *args_v = nullptr;
    RWR_TRY(multi_pinned(0, need, &pin_v));
    RWR_TRY(multi_pinned(1, sizeof(BuildSmallArgs) * (size_t)count, &args_v));
    uint8_t *pin = static_cast<uint8_t *>(pin_v);
    BuildSmallArgs *h_args = static_cast<BuildSmallArgs *>(args_v);
    DevBuf<uint8_t> d_in;
    DevBuf<BuildSmallArgs> d_args;
    RWR_TRY(d_in.alloc(in_bytes));
    RWR_TRY(d_args.alloc((size_t)count));
    std::vector<SmallBuild> builds((size_t)count);
#ifdef RWR_EXPERIMENTS
    static const bool mt_on = [] { const char *e = getenv("RWR_X_MULTI_TIMING"); return e && atoi(e) != 0; }();
    double mt0 = Stamps::now(), mt1 = 0, mt2 = 0, mt3 = 0, mt4 = 0, mt_up = 0, mt_begin = 0;
#endif
    for (int32_t i = 0; i < count; ++i) {
        rwr_graph *g = gs[i];
        g->sm_stage = pin + in_off[i];
        g->sm_out = pin + in_bytes + out_off[i];
        g->stage_dev_ext = d_in.p + in_off[i];
        const rwr_graph_desc &D = descs[i];
#ifdef RWR_EXPERIMENTS
        const double u0 = Stamps::now();
#endif
        RWR_TRY(graph_build_upload(g, D.node_id, D.node_type, D.rowptr, D.dst, D.etype, D.w));
        if (!small_build_ok(g)) { set_error("graphs_build_multi: graph %d does not qualify for the one-launch build", caller_index[i]); return RWR_E_INVALID; }
#ifdef RWR_EXPERIMENTS
        const double u1 = Stamps::now();
        mt_up += u1 - u0;
#endif
        RWR_TRY(small_build_begin(g, true, builds[i]));
#ifdef RWR_EXPERIMENTS
        mt_begin += Stamps::now() - u1;
#endif
        h_args[i] = builds[i].a;
    }
#ifdef RWR_EXPERIMENTS
    mt1 = Stamps::now();
#endif
    RWR_HIP(hipMemcpyAsync(d_in.p, pin, in_bytes, hipMemcpyHostToDevice, s));
    RWR_HIP(hipMemcpyAsync(d_args.p, h_args, sizeof(BuildSmallArgs) * (size_t)count, hipMemcpyHostToDevice, s));
    RWR_TRY(launch_build_small_multi(d_args.p, count, s));
#ifdef RWR_EXPERIMENTS
    mt2 = Stamps::now();
#endif
    RWR_HIP(hipStreamSynchronize(s));
#ifdef RWR_EXPERIMENTS
    mt3 = Stamps::now();
#endif
    for (int32_t i = 0; i < count; ++i) {
        rwr_graph *g = gs[i];
        const int32_t rc = small_build_end(g, builds[i], nullptr, nullptr);
        g->sm_stage = nullptr;            // (the arena belongs to the thread, not to the handle)
        g->sm_out = nullptr;
        g->stage_dev_ext = nullptr;
        g->staged = 0;                    // an incremental rebuild of this handle, should one follow, takes the general build
        if (rc != RWR_OK) {
            char msg[512];
            snprintf(msg, sizeof(msg), "%s", rwr_last_error());
            set_error("graph %d of the batch: %s", caller_index[i], msg);
            return rc;
        }
    }
#ifdef RWR_EXPERIMENTS
    mt4 = Stamps::now();
    if (mt_on)
        fprintf(stderr, "[multi build] %d graphs: prep %.0f us (upload %.0f, begin %.0f), enqueue %.0f, wait %.0f, finish %.0f\n", count, mt1 - mt0,
                mt_up, mt_begin, mt2 - mt1, mt3 - mt2, mt4 - mt3);
#endif
    return RWR_OK;
}

}  // namespace rwr
