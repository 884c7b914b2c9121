// K personalised walks ranked among the nodes of ONE node type (rwr_recommend_typed_batch): "who to follow"
// (candidates USER, the seed's FRIENDSHIP / FOLLOW targets and the seed itself left out), "similar items" (candidates ITEM
// from an item seed, nothing left out) and every other combination of a candidate type and a set of edge types.
//
// The walk is model.hip's batch of personalised Models in iteration mode: seeds dealt to tile slots, T WHOLE steps per tile
// group (GroupIter with a plan that reads the ranks, not the ITEM ranking: no tail row lists, no frontier lists, no fused or
// pruned last step -- those skip rows that only an ITEM ranking never reads).  The end of a group is recommend.hip's with
// both ITEM / LIKE constants turned into arguments:
//   - the exclusion marks the targets of the seed's raw links whose type has its bit in the mask (k_exclude_typed, over the
//     segments exclude_plan.h cuts the seeds' raw lists into) and, on request, the seed's own row (k_exclude_self: a seed
//     without raw links has no segment);
//   - the ranking is rank.hip's radix select over the candidate list of the type (top_n <= SEL_MAX_K).
// The candidate list is compacted on the device on first use and cached per handle (cand_plan.h: geometry and cache rule).
//
// rwr_recommend_typed_eval_batch is the same driver with the evaluating end: after the exclusion kernels the
// group is evaluated against the seeds' test sets by counting (eval_count.hip over the candidate list) instead of ranked, one
// record per seed leaves, and no list is written -- so top_n has no limit there.  The exclusion kernels serve
// rwr_recommend_restart_typed_batch as well (restart_batch.hip), through the launch_ wrappers below.
#include "eval_count.h"
#include "exclude_plan.h"
#include "iterate.h"

namespace rwr {

// ---- candidate rows of a node type: count per block, scan of the counts, ordered scatter (cand_plan.h) -------------------------

// does this thread's row match, and the wave's matches as a ballot; wc[w] = matches of wave w of the workgroup
__device__ __forceinline__ bool cand_match(int32_t n, const uint8_t *__restrict__ node_type, int32_t t, int32_t *wc,
                                           unsigned long long *bal)
{
    const int32_t b = blockIdx.x;
    const int32_t i = cand_block_lo(b) + (int32_t)threadIdx.x;
    const bool m = i < cand_block_hi(b, n) && node_type[i] == t;
    *bal = __ballot(m);
    if ((threadIdx.x & (WAVE - 1)) == 0) wc[threadIdx.x / WAVE] = __popcll(*bal);
    __syncthreads();
    return m;
}

__global__ __launch_bounds__(CAND_BLOCK) void k_cand_count(int32_t n, const uint8_t *__restrict__ node_type, int32_t t,
                                                           int32_t *__restrict__ block_cnt)
{
    __shared__ int32_t wc[CAND_BLOCK / WAVE];
    unsigned long long bal;
    cand_match(n, node_type, t, wc, &bal);
    if (threadIdx.x == 0) {
        int32_t c = 0;
        for (int w = 0; w < CAND_BLOCK / WAVE; ++w) c += wc[w];
        block_cnt[blockIdx.x] = c;
    }
}

// one workgroup: off[0 .. nb) from counts to exclusive offsets in place, off[nb] = their sum
__global__ __launch_bounds__(CAND_SCAN_CHUNK) void k_cand_scan(int32_t nb, int32_t *__restrict__ off)
{
    __shared__ int32_t wsum[CAND_SCAN_CHUNK / WAVE];
    __shared__ int32_t carry_s;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wv = tid / WAVE;
    if (tid == 0) carry_s = 0;
    __syncthreads();
    for (int32_t c0 = 0; c0 < nb; c0 += CAND_SCAN_CHUNK) {
        const int32_t b = c0 + tid;
        const int32_t cnt = b < nb ? off[b] : 0;
        int32_t inc = cnt;                                       // inclusive scan inside the wave
        for (int o = 1; o < WAVE; o <<= 1) {
            const int32_t v = __shfl_up(inc, o);
            if (lane >= o) inc += v;
        }
        if (lane == WAVE - 1) wsum[wv] = inc;
        __syncthreads();
        int32_t base = carry_s;
        for (int q = 0; q < wv; ++q) base += wsum[q];
        if (b < nb) off[b] = base + inc - cnt;
        __syncthreads();                                         // (every thread has read carry_s)
        if (tid == CAND_SCAN_CHUNK - 1) carry_s = base + inc;
        __syncthreads();
    }
    if (tid == 0) off[nb] = carry_s;
}

__global__ __launch_bounds__(CAND_BLOCK) void k_cand_scatter(int32_t n, const uint8_t *__restrict__ node_type, int32_t t,
                                                             const int32_t *__restrict__ off, int32_t total,
                                                             int32_t *__restrict__ rows)
{
    __shared__ int32_t wc[CAND_BLOCK / WAVE];
    unsigned long long bal;
    if (!cand_match(n, node_type, t, wc, &bal)) return;
    const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
    int32_t pos = off[blockIdx.x];
    for (int q = 0; q < wv; ++q) pos += wc[q];
    pos += __popcll(bal & ((1ull << lane) - 1ull));
    if (pos < total) rows[pos] = cand_block_lo(blockIdx.x) + (int32_t)threadIdx.x;
}

// The candidate list of node type `type` on the handle's current node set: the cached one, or built now into the entry
// cand_cache_choose names.  The stream is idle on entry (every entry point ends synchronised) and on return.
int32_t cand_rows_get(rwr_graph *g, int32_t type, const int32_t **rows, int32_t *nrows)
{
    const CandChoice ch = cand_cache_choose(g->cand_entry, type, g->n);
    CandEntry &e = g->cand_entry[ch.entry];
    DevBuf<int32_t> &list = g->cand_rows[ch.entry];
    ++g->cand_calls;
    if (!ch.hit) {
        e = CandEntry{};                                         // (a failure below leaves the entry empty)
        list.release();
        hipStream_t s = g->stream;
        const int32_t n = g->n, nb = cand_blocks(n);
        DevBuf<int32_t> off;
        RWR_TRY(off.alloc((size_t)nb + 1));
        int32_t total = 0;
        RWR_TRY(idle_on_error(s, [&]() -> int32_t {
            if (nb > 0) hipLaunchKernelGGL(k_cand_count, dim3((unsigned)nb), dim3(CAND_BLOCK), 0, s, n, g->node_type.p, type, off.p);
            hipLaunchKernelGGL(k_cand_scan, dim3(1), dim3(CAND_SCAN_CHUNK), 0, s, nb, off.p);
            RWR_HIP(hipGetLastError());
            RWR_HIP(hipMemcpyAsync(&total, off.p + nb, sizeof(int32_t), hipMemcpyDeviceToHost, s));
            RWR_HIP(hipStreamSynchronize(s));
            RWR_TRY(list.alloc((size_t)total));
            if (total > 0)
                hipLaunchKernelGGL(k_cand_scatter, dim3((unsigned)nb), dim3(CAND_BLOCK), 0, s, n, g->node_type.p, type, off.p, total,
                                   list.p);
            RWR_HIP(hipGetLastError());
            RWR_HIP(hipStreamSynchronize(s));                    // (off goes back to the block cache on return)
            return RWR_OK;
        }));
        e.type = type, e.n = n, e.rows = total;
    }
    e.used = g->cand_calls;
    *rows = list.p;
    *nrows = e.rows;
    return RWR_OK;
}

// ---- the exclusion ---------------------------------------------------------------------------------------------------------

// Recommender.cs:20-24 with the link type as a set: the targets of the seed's RAW out-links whose type has its bit in `mask`
// are not candidates.  One wave per segment of at most EXCLUDE_SEG_MAX links (exclude_plan.h), the lanes at consecutive links;
// a target of another node type receives a -1 that nobody reads.  Link types are as unchecked as node types, so a raw link may
// carry any value up to 255: the mask has no bit for a type >= TYPED_EDGE_TYPES, such a link is never masked, and the test
// in front of the shift keeps the shift count below the mask's width.
__global__ __launch_bounds__(64) void k_exclude_typed(int32_t n, int G, int32_t nseg, const int32_t *__restrict__ seg_slot,
                                                      const int64_t *__restrict__ seg_p0, const int64_t *__restrict__ seg_p1,
                                                      const int32_t *__restrict__ dst, const uint8_t *__restrict__ etype,
                                                      uint32_t mask, double *__restrict__ X)
{
    const int32_t j = blockIdx.x;
    if (j >= nseg) return;
    const int32_t q = seg_slot[j];
    double *x = X + (size_t)(q / G) * (size_t)n * G + (q % G);
    const int64_t p1 = seg_p1[j];
    for (int64_t p = seg_p0[j] + threadIdx.x; p < p1; p += WAVE) {
        const uint32_t t = etype[p];                             // (unchecked at create: any value 0..255)
        if (t < TYPED_EDGE_TYPES && ((mask >> t) & 1u)) x[(size_t)dst[p] * G] = -1.0;
    }
}

// exclude_self: one thread per slot marks the seed's own row -- also of a seed without raw links, which has no segment
__global__ __launch_bounds__(64) void k_exclude_self(int32_t n, int G, int nslots, const int32_t *__restrict__ seeds,
                                                     double *__restrict__ X)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nslots) return;
    const int32_t s = seeds[q];
    if (s < 0) return;
    X[(size_t)(q / G) * (size_t)n * G + (size_t)s * G + (q % G)] = -1.0;
}

void launch_exclude_typed(rwr_graph *g, int G, int32_t nseg, const int32_t *seg_slot, const int64_t *seg_p0, const int64_t *seg_p1,
                          uint32_t mask, double *X, hipStream_t s)
{
    if (nseg <= 0 || mask == 0) return;
    hipLaunchKernelGGL(k_exclude_typed, dim3((unsigned)nseg), dim3(64), 0, s, g->n, G, nseg, seg_slot, seg_p0, seg_p1, g->dst.p,
                       g->etype.p, mask, X);
}

// exclude_members (rwr_recommend_restart_typed_batch): one thread per (slot, member) pair of the group (member_plan.h) marks
// the member's own row in its vector's column -- also of a member without raw links.  A member listed twice, or that is a
// masked target as well, simply receives its -1 twice.
__global__ __launch_bounds__(256) void k_exclude_members(int32_t n, int G, int32_t npairs, const int32_t *__restrict__ pair_slot,
                                                         const int32_t *__restrict__ pair_row, double *__restrict__ X)
{
    const int32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= npairs) return;
    const int32_t q = pair_slot[j], row = pair_row[j];
    if (row < 0 || row >= n) return;                             // (member_plan.h plans rows of [0, n) only)
    X[(size_t)(q / G) * (size_t)n * G + (size_t)row * G + (q % G)] = -1.0;
}
void launch_exclude_members(rwr_graph *g, int G, int32_t npairs, const int32_t *pair_slot, const int32_t *pair_row, double *X,
                            hipStream_t s)
{
    if (npairs <= 0) return;
    hipLaunchKernelGGL(k_exclude_members, dim3(cdiv((size_t)npairs, 256)), dim3(256), 0, s, g->n, G, npairs, pair_slot, pair_row, X);
}

// ---- the driver --------------------------------------------------------------------------------------------------------------

// ev != nullptr: the evaluating form -- no list tables, the group's end is eval_group, K records leave
static int32_t typed_body(rwr_graph *g, const int32_t *seeds, int32_t K, double d, int32_t n_iter, int32_t top_n,
                          int32_t cand_type, uint32_t mask, int32_t exclude_self, int64_t *ids, double *scores, int32_t *counts,
                          EvalEnd *ev, const char *who)
{
    const double t_begin = now_ms();
    const int64_t T = n_iter;
    hipStream_t s = g->stream;
    const int32_t *rows = nullptr;
    int32_t nrows = 0;
    RWR_TRY(cand_rows_get(g, cand_type, &rows, &nrows));         // (before the workspace is sized from what is free)
    const int G = resolve_G(g, K);
    int TG = 1;
    RWR_TRY(ensure_workspace(g, G, K, &TG));
    const int ntiles = (int)cdiv((size_t)K, (size_t)G);
    std::vector<int32_t> slot_k;
    RWR_TRY(upload_seed_slots(g, seeds, K, G, &slot_k));

    // the seeds' raw lists cut into segments: set k = {seeds[k]}.  Mask 0 looks at no link.
    ExcludePlan plan;
    DevBuf<int32_t> d_seg_slot;
    DevBuf<int64_t> d_seg_p0, d_seg_p1;
    StreamsIdle idle{g};                                         // (the plan's device copy outlives the kernels that read it)
    size_t nseg_all = 0;
    if (mask != 0) {
        std::vector<int64_t> set_ptr((size_t)K + 1);
        for (int32_t k = 0; k <= K; ++k) set_ptr[(size_t)k] = k;
        plan = exclude_plan(g->n, g->h_rowptr.data(), slot_k.size(), slot_k.data(), (size_t)TG * G, K, set_ptr.data(), seeds);
        if (plan.check.verdict != EXCLUDE_OK) {                  // (the seeds were checked before the call got here)
            set_error("%s: the seeds failed the exclusion plan's check (verdict %d)", who, (int)plan.check.verdict);
            return RWR_E_INVALID;
        }
        nseg_all = plan.seg_slot.size();
        if (nseg_all > 0x7FFFFFFFull) { set_error("%s: too many exclusion segments", who); return RWR_E_UNSUPPORTED; }
    }
    if (nseg_all > 0) {
        RWR_TRY(d_seg_slot.alloc(nseg_all));
        RWR_TRY(d_seg_p0.alloc(nseg_all));
        RWR_TRY(d_seg_p1.alloc(nseg_all));
        RWR_HIP(hipMemcpyAsync(d_seg_slot.p, plan.seg_slot.data(), nseg_all * sizeof(int32_t), hipMemcpyHostToDevice, s));
        RWR_HIP(hipMemcpyAsync(d_seg_p0.p, plan.seg_p0.data(), nseg_all * sizeof(int64_t), hipMemcpyHostToDevice, s));
        RWR_HIP(hipMemcpyAsync(d_seg_p1.p, plan.seg_p1.data(), nseg_all * sizeof(int64_t), hipMemcpyHostToDevice, s));
    }
    if (ev) RWR_TRY(eval_prepare(g, *ev, K, slot_k, (size_t)TG * G, who, s));
    else RWR_TRY(ensure_out_tables(g, K, top_n, s));

    Profile prof(g);
    for (int t0 = 0, grp = 0; t0 < ntiles; t0 += TG, ++grp) {
        const int tg = (ntiles - t0 < TG) ? (ntiles - t0) : TG;
        const size_t q0 = (size_t)t0 * G;
        const int32_t *dseeds = g->d_seeds.p + q0;
        GroupIter gi(g, G, tg, dseeds, g->d_evoff.p + q0, d);
        hipEvent_t i0; RWR_TRY(prof.record(i0, s));
        RWR_TRY(gi.init(true, true, /*ranking_only=*/false));    // Model ctor; every step writes every row
        while (gi.it < T) RWR_TRY(gi.step(plan_step(gi.cfg, gi.it, T), prof));   // deliverRanks + updateRanks
        RWR_TRY(prof.end(prof.iter, i0, s));
        int32_t real = 0;
        for (size_t q = q0; q < q0 + (size_t)tg * G; ++q) real += slot_k[q] >= 0;
        g->stats.spmm_seed_steps += (int64_t)real * (T > 0 ? T : 0);
        g->stats.spmm_dense_seed_steps += (int64_t)real * gi.dense_steps;

        hipEvent_t a; RWR_TRY(prof.record(a, s));
        if (mask != 0) {
            const int64_t j0 = plan.group_off[(size_t)grp], nseg = plan.group_off[(size_t)grp + 1] - j0;
            if (nseg > 0)
                hipLaunchKernelGGL(k_exclude_typed, dim3((unsigned)nseg), dim3(64), 0, s, g->n, G, (int32_t)nseg, d_seg_slot.p + j0,
                                   d_seg_p0.p + j0, d_seg_p1.p + j0, g->dst.p, g->etype.p, mask, gi.X);
        }
        if (exclude_self)
            hipLaunchKernelGGL(k_exclude_self, dim3(cdiv((size_t)tg * G, 64)), dim3(64), 0, s, g->n, G, tg * G, dseeds, gi.X);
        RWR_HIP(hipGetLastError());
        if (ev) RWR_TRY(eval_group(g, *ev, G, tg, q0, gi.X, rows, nrows, s));   // (no candidate: the zeroed records stand)
        else if (nrows > 0) RWR_TRY(rank_group_select(g, G, tg, g->d_slot_k.p + q0, top_n, gi.X, dseeds, s, rows, nrows));
        RWR_TRY(prof.end(prof.rank, a, s));
    }
    if (ev) RWR_TRY(eval_copy_back(g, *ev, K, who, s));
    else RWR_TRY(copy_lists_back(g, K, top_n, ids, scores, counts, top_n));
    g->stats.seeds_done += K;
    return finish_model_batch(g, prof, G, TG, t_begin);
}

int32_t recommend_typed_batch(rwr_graph *g, const int32_t *seeds, int32_t K, double d, int32_t n_iter, int32_t top_n,
                              int32_t cand_type, uint32_t excl_edge_mask, int32_t exclude_self, int64_t *ids, double *scores,
                              int32_t *counts)
{
    static const char *const who = "rwr_recommend_typed_batch";
    return no_throw(who, [&] {
        return typed_body(g, seeds, K, d, n_iter, top_n, cand_type, excl_edge_mask, exclude_self, ids, scores, counts, nullptr, who);
    });
}

int32_t recommend_typed_eval_batch(rwr_graph *g, const int32_t *seeds, int32_t K, double d, int32_t n_iter, int32_t top_n,
                                   int32_t cand_type, uint32_t excl_edge_mask, int32_t exclude_self, const int64_t *test_ptr,
                                   const int64_t *test_ids, int64_t *n_hits, double *sum_precision, int64_t *list_len)
{
    static const char *const who = "rwr_recommend_typed_eval_batch";
    EvalEnd ev;                                                  // (declared before the body's StreamsIdle: the buffers outlive the kernels)
    ev.test_ptr = test_ptr, ev.test_ids = test_ids, ev.top_n = top_n;
    ev.n_hits = n_hits, ev.sum_precision = sum_precision, ev.list_len = list_len;
    return no_throw(who, [&] {
        return typed_body(g, seeds, K, d, n_iter, top_n, cand_type, excl_edge_mask, exclude_self, nullptr, nullptr, nullptr, &ev, who);
    });
}

}  // namespace rwr
