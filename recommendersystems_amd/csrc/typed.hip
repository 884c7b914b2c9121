// K personalised walks ranked among the nodes of ONE node type (rwr_recommend_typed_batch): "who to follow"
// (candidates USER, the seed's FRIENDSHIP / FOLLOW targets and the seed itself left out), "similar items" (candidates ITEM
// from an item seed, nothing left out) and every other combination of a candidate type and a set of edge types.
//
// The walk is model.hip's batch of personalised Models in iteration mode: seeds dealt to tile slots, T WHOLE steps per tile
// group (GroupIter with a plan that reads the ranks, not the ITEM ranking: no tail row lists, no frontier lists, no fused or
// pruned last step -- those skip rows that only an ITEM ranking never reads).  The end of a group is a RankedEnd
// (ranked_end.h), recommend.hip's end with both ITEM / LIKE constants turned into arguments:
//   - the exclusion sets are the singletons {seed}: the targets of the seed's raw links whose type has its bit in the mask
//     are marked and, on request, the seed's own row (named by slot: d_seeds);
//   - the ranking is rank.hip's radix select over the candidate list of the type (top_n <= SEL_MAX_K).
// The candidate list is compacted on the device on first use and cached per handle (cand_plan.h: geometry and cache rule);
// rwr_recommend_restart_typed_batch (restart_batch.hip) ranks over the same lists.
//
// rwr_recommend_typed_eval_batch is the same driver with the evaluating destination: after the exclusion the
// group is evaluated against the seeds' test sets by counting (eval_count.hip over the candidate list) instead of ranked, one
// record per seed leaves, and no list is written -- so top_n has no limit there.  rwr_recommend_typed_positions_batch
//  is the third destination: the same counting, the position and score of every test id in the whole list.
//
// rwr_recommend_filtered_batch and rwr_recommend_filtered_positions_batch (filter.hip) run this driver with a
// pool or deny lists in their TypedCall (typed_call.h): the candidates narrowed to the caller's pool, the seeds' deny lists
// marked after the link exclusion.  rwr_recommend_capped_batch and rwr_recommend_capped_positions_batch (group_cap.hip,
// DESIGN.md 3.21) add group labels, from which a GroupCap joins the end: built here once the candidate list exists, applied
// by the end after the deny marks.  rwr_recommend_explained_batch (explain.hip) adds a WhyEnd: the end then
// also reads the group's previous ranks.  rwr_recommend_long_batch (long_list.hip) is the explained entry without
// reasons up to the select's limit and names a LongEnd beyond it.  All nine entries come in through the one typed_body().
#include "explain.h"
#include "filter.h"
#include "group_cap.h"
#include "long_list.h"
#include "node_remove_plan.h"   // (nrm_wave_count, nrm_rank_in_chunk: a match's position inside its workgroup)

namespace rwr {

// ---- candidate rows: count per block, scan of the counts, ordered scatter (cand_plan.h, filter_plan.h) -------------------------
// One compaction for the handle's per-type lists (no bitmap) and a call's own list (the pool's bitmap, any type).

// does this thread's row match, and the wave's matches as a ballot; wc[w] = matches of wave w of the workgroup
__device__ __forceinline__ bool cand_match(int32_t n, const uint8_t *__restrict__ node_type, int32_t t,
                                           const uint32_t *__restrict__ bitmap, int32_t *wc, unsigned long long *bal)
{
    const int32_t b = blockIdx.x;
    const int32_t i = cand_block_lo(b) + (int32_t)threadIdx.x;
    const bool m = i < cand_block_hi(b, n) && filter_match(node_type, t, bitmap, i);
    *bal = __ballot(m);
    if ((threadIdx.x & (WAVE - 1)) == 0) wc[threadIdx.x / WAVE] = nrm_wave_count(*bal);
    __syncthreads();
    return m;
}

__global__ __launch_bounds__(CAND_BLOCK) void k_cand_count(int32_t n, const uint8_t *__restrict__ node_type, int32_t t,
                                                           const uint32_t *__restrict__ bitmap, int32_t *__restrict__ block_cnt)
{
    __shared__ int32_t wc[CAND_BLOCK / WAVE];
    unsigned long long bal;
    cand_match(n, node_type, t, bitmap, wc, &bal);
    if (threadIdx.x == 0) {
        int32_t c = 0;
        for (int w = 0; w < CAND_BLOCK / WAVE; ++w) c += wc[w];
        block_cnt[blockIdx.x] = c;
    }
}

// THE workgroup scan of the library's compactions: one workgroup, off[0 .. nb) from counts to exclusive offsets in place,
// off[nb] = their sum.  T = int32_t for lists of rows (here, group_cap.hip, node_remove.hip's ITEM orders), int64_t for the
// link chunks of node_remove.hip: a graph has up to 2^32-2 links.
template <typename T>
__global__ __launch_bounds__(CAND_SCAN_CHUNK) void k_cand_scan(T nb, T *__restrict__ off)
{
    __shared__ T wsum[CAND_SCAN_CHUNK / WAVE];
    __shared__ T carry_s;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wv = tid / WAVE;
    if (tid == 0) carry_s = 0;
    __syncthreads();
    for (T c0 = 0; c0 < nb; c0 += CAND_SCAN_CHUNK) {
        const T b = c0 + tid;
        const T cnt = b < nb ? off[b] : 0;
        T inc = cnt;                                             // inclusive scan inside the wave
        for (int o = 1; o < WAVE; o <<= 1) {
            const T v = __shfl_up(inc, o);
            if (lane >= o) inc += v;
        }
        if (lane == WAVE - 1) wsum[wv] = inc;
        __syncthreads();
        T base = carry_s;
        for (int q = 0; q < wv; ++q) base += wsum[q];
        if (b < nb) off[b] = base + inc - cnt;
        __syncthreads();                                         // (every thread has read carry_s)
        if (tid == CAND_SCAN_CHUNK - 1) carry_s = base + inc;
        __syncthreads();
    }
    if (tid == 0) off[nb] = carry_s;
}

__global__ __launch_bounds__(CAND_BLOCK) void k_cand_scatter(int32_t n, const uint8_t *__restrict__ node_type, int32_t t,
                                                             const uint32_t *__restrict__ bitmap, const int32_t *__restrict__ off,
                                                             int32_t total, int32_t *__restrict__ rows)
{
    __shared__ int32_t wc[CAND_BLOCK / WAVE];
    unsigned long long bal;
    if (!cand_match(n, node_type, t, bitmap, wc, &bal)) return;
    const int32_t pos = off[blockIdx.x] + nrm_rank_in_chunk(0, wc, threadIdx.x / WAVE, bal, threadIdx.x & (WAVE - 1));
    if (pos >= 0 && pos < total) rows[pos] = cand_block_lo(blockIdx.x) + (int32_t)threadIdx.x;
}

// ... for every other compaction as well (filter.h)
void launch_cand_scan(int32_t nb, int32_t *off, hipStream_t s)
{
    hipLaunchKernelGGL(k_cand_scan<int32_t>, dim3(1), dim3(CAND_SCAN_CHUNK), 0, s, nb, off);
}
void launch_cand_scan(int64_t nb, int64_t *off, hipStream_t s)
{
    hipLaunchKernelGGL(k_cand_scan<int64_t>, dim3(1), dim3(CAND_SCAN_CHUNK), 0, s, nb, off);
}

int32_t cand_compact(rwr_graph *g, int32_t type, const uint32_t *bitmap, int32_t *off, DevBuf<int32_t> &list, int32_t *nrows)
{
    hipStream_t s = g->stream;
    const int32_t n = g->n, nb = cand_blocks(n);
    int32_t total = 0;
    if (nb > 0) hipLaunchKernelGGL(k_cand_count, dim3((unsigned)nb), dim3(CAND_BLOCK), 0, s, n, g->node_type.p, type, bitmap, off);
    launch_cand_scan(nb, off, s);
    RWR_HIP(hipGetLastError());
    RWR_HIP(hipMemcpyAsync(&total, off + nb, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    RWR_HIP(hipStreamSynchronize(s));
    if (total < 0 || total > n) { set_error("candidate list build: %d rows of %d", total, n); return RWR_E_HIP; }
    RWR_TRY(list.alloc((size_t)total));
    if (total > 0)
        hipLaunchKernelGGL(k_cand_scatter, dim3((unsigned)nb), dim3(CAND_BLOCK), 0, s, n, g->node_type.p, type, bitmap, off, total, list.p);
    RWR_HIP(hipGetLastError());
    *nrows = total;
    return RWR_OK;
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
        DevBuf<int32_t> off;
        RWR_TRY(off.alloc((size_t)cand_blocks(g->n) + 1));
        int32_t total = 0;
        RWR_TRY(idle_on_error(g->stream, [&]() -> int32_t {
            RWR_TRY(cand_compact(g, type, nullptr, off.p, list, &total));
            RWR_HIP(hipStreamSynchronize(g->stream));            // (off goes back to the block cache on return)
            return RWR_OK;
        }));
        e.type = type, e.n = g->n, e.rows = total;
    }
    e.used = g->cand_calls;
    *rows = list.p;
    *nrows = e.rows;
    return RWR_OK;
}

// ---- the driver --------------------------------------------------------------------------------------------------------------

// The one driver of the eight seed-driven typed entries: `call` as typed_call_check passed it, a nonneg graph, d in [0, 1],
// n_iter >= 0.  The candidates and the exclusion: the list of cand_type, the sets {seeds[k]}, the mask, and the seeds' own
// rows on request (a seed without raw links has no link to mark it by).  A pool or cand_type FILTER_ANY_TYPE puts the call's
// own list (filter_rows_build) in the place of the handle's cached one, which is then neither read nor evicted; the deny
// lists go to the end as its second set description.  group_of != nullptr: the cap's tables are built from whichever list
// serves the call -- the cached one is only read.  Reasons: only when something of them is asked for -- with n_why == 0 and
// neither nodes nor why_total the explained entry is the capped one, launch for launch.
int32_t typed_body(rwr_graph *g, const TypedCall &call, double d, int32_t n_iter, const char *who)
{
    const double t_begin = now_ms();
    const int64_t T = n_iter;
    const int32_t K = call.K;
    hipStream_t s = g->stream;
    // (the end and what it points to are declared before idle: ranked_end.h's lifetime rule)
    GroupCap cap;
    cap.group_of = call.group_of, cap.m = call.group_cap;
    WhyEnd why;
    why.n_why = call.n_why, why.T = T, why.c1 = 1 - d;           // (GroupIter's c1: Model.cs:84)
    why.nodes = call.nodes, why.why_src = call.why_src, why.why_term = call.why_term, why.why_total = call.why_total;
    LongEnd lng;
    lng.nodes = call.nodes;
    EvalEnd ev;
    ev.test_ptr = call.test_ptr, ev.test_ids = call.test_ids, ev.top_n = call.top_n;
    ev.n_hits = call.n_hits, ev.sum_precision = call.sum_precision, ev.list_len = call.list_len;
    PosEnd pe;
    pe.ev.test_ptr = call.test_ptr, pe.ev.test_ids = call.test_ids;
    pe.pos_out = call.pos_out, pe.score_out = call.score_out, pe.list_len = call.list_len;
    RankedEnd end;
    end.who = who;
    if (call.dest == CALL_LISTS) {
        end.top_n = call.top_n, end.ids = call.ids, end.scores = call.scores, end.counts = call.counts;
        if (long_applies(call.top_n)) end.lng = &lng;            // (only the long entry's ladder lets such a top_n through)
        else if (call.n_why > 0 || call.nodes || call.why_total) end.why = &why;
    } else if (call.dest == CALL_EVAL) {
        end.ev = &ev;
    } else {
        end.pos = &pe;
    }
    if (call.group_of) end.cap = &cap;
    end.deny_ptr = call.deny_ptr, end.deny_idx = call.deny_idx;

    Profile prof(g);
    DevBuf<int32_t> own_rows;                                    // (declared before idle: released after the call's last synchronisation)
    // (either list before the workspace is sized from what is free)
    if (call.pool_count >= 0 || call.cand_type == FILTER_ANY_TYPE) {
        RWR_TRY(filter_rows_build(g, call.cand_type, call.pool_count, call.pool_idx, own_rows, &end.nrows, prof));
        end.rows = own_rows.p;
    } else {
        RWR_TRY(cand_rows_get(g, call.cand_type, &end.rows, &end.nrows));
    }
    const int G = resolve_G(g, K);
    int TG = 1;
    if (end.cap) {                                               // (a tile group holds at most this many tiles: ensure_workspace)
        const int ntiles_all = (int)cdiv((size_t)K, (size_t)G), most = g->opts.tile_group > 0 ? g->opts.tile_group : 192;
        RWR_TRY(cap_build(g, cap, end.rows, end.nrows, G, ntiles_all < most ? ntiles_all : most, prof));
    }
    RWR_TRY(ensure_workspace(g, G, K, &TG));
    const int ntiles = (int)cdiv((size_t)K, (size_t)G);
    std::vector<int32_t> slot_k;
    RWR_TRY(upload_seed_slots(g, call.seeds, K, G, &slot_k));

    // set k = {seeds[k]}, its one member per slot in d_seeds
    std::vector<int64_t> set_ptr((size_t)K + 1);
    for (int32_t k = 0; k <= K; ++k) set_ptr[(size_t)k] = k;
    end.set_ptr = set_ptr.data(), end.set_idx = call.seeds;
    end.mask = call.excl_edge_mask, end.members = call.exclude_self != 0, end.slot_member = g->d_seeds.p;
    StreamsIdle idle{g};                                         // (declared after end: ranked_end.h)
    RWR_TRY(end.prepare(g, K, slot_k, (size_t)TG * G, s));

    for (int t0 = 0, grp = 0; t0 < ntiles; t0 += TG, ++grp) {
        const int tg = (ntiles - t0 < TG) ? (ntiles - t0) : TG;
        const size_t q0 = (size_t)t0 * G;
        GroupIter gi(g, G, tg, g->d_seeds.p + q0, g->d_evoff.p + q0, d);
        hipEvent_t i0; RWR_TRY(prof.record(i0, s));
        RWR_TRY(gi.init(true, true, /*ranking_only=*/false));    // Model ctor; every step writes every row
        while (gi.it < T) RWR_TRY(gi.step(plan_step(gi.cfg, gi.it, T), prof));   // deliverRanks + updateRanks
        RWR_TRY(prof.end(prof.iter, i0, s));
        int32_t real = 0;
        for (size_t q = q0; q < q0 + (size_t)tg * G; ++q) real += slot_k[q] >= 0;
        g->stats.spmm_seed_steps += (int64_t)real * (T > 0 ? T : 0);
        g->stats.spmm_dense_seed_steps += (int64_t)real * gi.dense_steps;
        RWR_TRY(end.finish_group(g, G, tg, grp, q0, gi.X, prof, s, gi.Y));   // (Y: the ranks the last step read, whole)
    }
    RWR_TRY(end.copy_back(g, K));
    g->stats.seeds_done += K;
    return finish_model_batch(g, prof, G, TG, t_begin);
}

}  // namespace rwr

