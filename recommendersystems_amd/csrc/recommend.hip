// Recommender.Recommendation for a batch of seeds (rwr_recommend_batch and the entry points built on it): sizes the
// workspace, deals the seeds to tiles and tile groups, runs each group's power iteration (iterate.hip: iterate_group), then
// the exclusion and the ranking (rank.h), and copies the lists back.
#include "iterate.h"
#include "seed_row.h"

#include <algorithm>
#include <chrono>

namespace rwr {

int resolve_G(const rwr_graph *g, int32_t K)
{
    int G = g->opts.tile_seeds;
    if (G == 1 || G == 2 || G == 4 || G == 8 || G == 16 || G == 32 || G == 64) return G;
    // 32 seeds per tile (256-byte rows) measured best on the 100M-link graph: half the matrix re-streaming and
    // half the per-entry instruction work of 16, while 64 gains nothing more and lengthens the seed-row chain
    // (on the 20M-link graph 16 is a little faster: the ranking stage scales with the tile width)
    // ... and 32 again wins on dense graphs (hundreds of links per node: the MovieLens-shaped config, +10 %)
    const int cap = (g->n >= spmv_big_n() || g->nnz / (g->n > 0 ? g->n : 1) >= 64) ? 32 : 16;
    int want = 1;
    while (want < K && want < cap) want <<= 1;
    return want;
}

// extra_mats (rwr_model_run_batch: the difference / staging matrix in g->cs_diff) is counted in the sizing so that a large
// graph shrinks the tile group instead of failing
int32_t ensure_workspace(rwr_graph *g, int G, int32_t K, int *TG_out, int extra_mats)
{
    const size_t n = (size_t)g->n;
    const int ntiles = (int)cdiv((size_t)K, (size_t)G);
    // a model batch's difference / staging matrix (TG * n * G doubles) is given back before a call that needs none sizes its
    // tile group, instead of holding memory that call would count as taken (model_run needs at most n of it, and re-takes them)
    // (the stream is idle: every entry point synchronises before it returns)
    if (!extra_mats && g->cs_diff.count > n) g->cs_diff.release();
    size_t cap = (size_t)g->opts.workspace_bytes;
    if (cap == 0) {
        size_t fr = 0, tot = 0;
        RWR_HIP(hipMemGetInfo(&fr, &tot));
        // what is already held by the rank matrices counts as available
        fr += (g->X.count + g->Y.count + g->Z0.count + g->Z1.count) * sizeof(double);
        if (extra_mats) fr += g->cs_diff.count * sizeof(double);
        // three quarters of what is free go to the rank matrices; the rest stays for the buffers sized after them (frontier
        // bitmaps and seed slots below -- inside the retry loop --, chain-scan cells, ranking keys) and for other handles
        cap = fr / 2 + fr / 4;
    }
    const size_t mats = (g->vf ? 4 : 2) + (size_t)extra_mats;   // X, Y (+ the value-free path's z of the current and of the next ranks)
    const size_t per_tile = mats * n * (size_t)G * sizeof(double);
    int TG = g->opts.tile_group > 0 ? g->opts.tile_group : (int)(cap / (per_tile ? per_tile : 1));
    if (TG < 1) TG = 1;
    if (TG > ntiles) TG = ntiles;
    if (TG > 65535 / G) TG = 65535 / G;   // grid.y of the per-slot kernels is TG * G
    // exact mode: every tile's chain workgroup must be resident beside the SpMM (one per CU, see k_gate in seed_chain.hip)
    if (g->opts.tile_group <= 0 && TG > 192) TG = 192;
    // the rank matrices: if the device cannot give what the sizing above asked for (other handles of the process -- the
    // reference runs up to ten host threads, Program.cs:11 -- may have taken their share since hipMemGetInfo was read),
    // halve the tile group and try again instead of failing the call
    for (;;) {
        int32_t rc = g->X.ensure((size_t)TG * n * G);
        if (rc == RWR_OK) rc = g->Y.ensure((size_t)TG * n * G);
        if (rc == RWR_OK && g->vf) {
            rc = g->Z0.ensure((size_t)TG * n * G);
            if (rc == RWR_OK) rc = g->Z1.ensure((size_t)TG * n * G);
        }
        if (rc == RWR_OK && extra_mats) rc = g->cs_diff.ensure((size_t)TG * n * G);
        if (rc == RWR_OK) rc = g->d_seeds.ensure((size_t)ntiles * G);
        if (rc == RWR_OK) rc = g->d_nz.ensure(3 * (size_t)TG * ((n + 31) / 32));   // X, Y non-zero rows + active destination rows
        if (rc == RWR_OK) rc = g->d_gate.ensure(64);
        if (rc == RWR_OK) break;
        if (rc != RWR_E_NOMEM || TG <= 1 || g->opts.tile_group > 0) return rc;
        (void)hipGetLastError();
        g->X.release(); g->Y.release(); g->Z0.release(); g->Z1.release(); g->d_nz.release();
        if (extra_mats) g->cs_diff.release();
        TG = (TG + 1) / 2;
    }
    *TG_out = TG;
    return RWR_OK;
}

// Seeds are dealt to tile slots by in-degree rank, round-robin over the tiles, so that the links INTO the
// seeds (the only non-streaming work of the exact seed-row kernel) spread evenly over the tiles instead of
// piling up in the tile that would hold the batch's hottest seeds.  slot_k maps a slot back to the
// caller's batch position; padding slots hold seed -1.  Also: offsets of every slot's in-link term list.
int32_t upload_seed_slots(rwr_graph *g, const int32_t *seeds, int32_t K, int G, std::vector<int32_t> *slot_k_out,
                          std::vector<int32_t> *slot_seed_out)
{
    const int ntiles = (int)cdiv((size_t)K, (size_t)G);
    const size_t slots = (size_t)ntiles * G;
    std::vector<int32_t> hs(slots, -1), sk(slots, -1);
    std::vector<int64_t> off(slots + 1, 0);
    std::vector<int32_t> order(K);
    for (int32_t k = 0; k < K; ++k) order[k] = k;
    auto indeg = [&](int32_t k) { return g->h_in_ptr[seeds[k] + 1] - g->h_in_ptr[seeds[k]]; };
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return indeg(a) > indeg(b); });
    for (int32_t r = 0; r < K; ++r) {
        const size_t slot = (size_t)(r % ntiles) * G + (size_t)(r / ntiles);
        hs[slot] = seeds[order[r]];
        sk[slot] = order[r];
    }
    for (size_t q = 0; q < slots; ++q) {
        int64_t deg = hs[q] >= 0 ? g->h_in_ptr[hs[q] + 1] - g->h_in_ptr[hs[q]] : 0;
        off[q + 1] = off[q] + deg;
    }
    RWR_TRY(g->d_seeds.ensure(slots));
    RWR_TRY(g->d_slot_k.ensure(slots));
    RWR_TRY(g->d_evoff.ensure(slots + 1));
    RWR_TRY(g->d_evterm.ensure((size_t)off[slots] + 1));
    RWR_HIP(hipMemcpy(g->d_seeds.p, hs.data(), slots * sizeof(int32_t), hipMemcpyHostToDevice));
    RWR_HIP(hipMemcpy(g->d_slot_k.p, sk.data(), slots * sizeof(int32_t), hipMemcpyHostToDevice));
    RWR_HIP(hipMemcpy(g->d_evoff.p, off.data(), (slots + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
    if (slot_k_out) *slot_k_out = sk;
    if (slot_seed_out) *slot_seed_out = hs;
    return RWR_OK;
}

double now_ms()
{
    using namespace std::chrono;
    return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

// The results of a call, K_all x top_n (device rows are top_n wide; host rows are row_stride wide), once the main stream
// has finished.  ids / scores NULL: the caller consumes the lists on the device (e.g. rwr_recommend_eval).
int32_t copy_lists_back(rwr_graph *g, int32_t K_all, int32_t top_n, int64_t *ids, double *scores, int32_t *counts,
                        int64_t row_stride)
{
    hipStream_t s = g->stream;
    std::vector<int32_t> hc((size_t)K_all);
    RWR_HIP(hipMemcpyAsync(hc.data(), g->d_counts.p, hc.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (ids && scores) {
        RWR_HIP(hipMemcpy2DAsync(ids, (size_t)row_stride * sizeof(int64_t), g->d_out_id.p, (size_t)top_n * sizeof(int64_t),
                                 (size_t)top_n * sizeof(int64_t), (size_t)K_all, hipMemcpyDeviceToHost, s));
        RWR_HIP(hipMemcpy2DAsync(scores, (size_t)row_stride * sizeof(double), g->d_out_score.p,
                                 (size_t)top_n * sizeof(double), (size_t)top_n * sizeof(double), (size_t)K_all,
                                 hipMemcpyDeviceToHost, s));
    }
    RWR_HIP(hipStreamSynchronize(s));
    for (int32_t k = 0; k < K_all; ++k) counts[k] = hc[k];
    return RWR_OK;
}

int32_t recommend_batch(rwr_graph *g, const int32_t *seeds, int32_t K, double d, int32_t n_iter, int32_t top_n,
                        int64_t *ids, double *scores, int32_t *counts, int64_t row_stride)
{
    const double t_begin = now_ms();
    const int32_t n = g->n;
    if (!g->nonneg) {
        // the exclusion marker (-1) and the ranking keys assume scores >= 0, i.e. weights >= 0 and finite row sums -- what
        // the reference's loader produces (DataLoader.cs:293-294,431-432).  Model.run still works on such a graph.
        set_error("Recommendation needs non-negative finite link weights and positive row sums (a raw weight is negative or "
                  "NaN, or the explicit weights of a node sum to 0 or overflow); rwr_model_run accepts such graphs");
        return RWR_E_UNSUPPORTED;
    }
    if (!(d >= 0.0 && d <= 1.0)) {
        // outside [0, 1] ranks go negative (or NaN): the exclusion marker and the ranking keys assume scores >= 0
        set_error("Recommendation needs a damping factor in [0, 1] (got %g); rwr_model_run accepts any value", d);
        return RWR_E_UNSUPPORTED;
    }
    for (int32_t k = 0; k < K; ++k)
        if (seeds[k] < 0 || seeds[k] >= n) {
            set_error("seed %d (batch position %d) is outside [0, %d)", seeds[k], k, n);
            return RWR_E_RANGE;
        }
    if (K == 1 && small_path_ok(g) && small_path_seed_ok(g, seeds[0])) {
        // ego-network-sized graph, one seed (the unmodified harness's call, Experiment.cs:109): the whole call is one launch
        RWR_TRY(recommend_small(g, seeds[0], d, n_iter, top_n, ids, scores, counts));
        g->stats.seeds_done += 1;
        g->stats.total_wall_ms += now_ms() - t_begin;
        return RWR_OK;
    }
    // dangling seeds (no explicit out-link) are answered directly (see k_emit_dangling); the rest is iterated
    const int32_t K_all = K;
    std::vector<int32_t> live_seeds, live_rows, dang_seeds, dang_rows;
    const bool shortcut = top_n <= rank_select_max_k() && K_all > 1;
    for (int32_t k = 0; k < K_all; ++k) {
        if (shortcut && g->h_dangling[seeds[k]]) { dang_seeds.push_back(seeds[k]); dang_rows.push_back(k); }
        else { live_seeds.push_back(seeds[k]); live_rows.push_back(k); }
    }
    const bool any_dangling = !dang_seeds.empty();
    if (any_dangling) { seeds = live_seeds.data(); K = (int32_t)live_seeds.size(); }
    hipStream_t s = g->stream;
    RWR_TRY(ensure_out_tables(g, K_all, top_n, s));
    if (K == 0) {   // every seed of the batch is dangling
        RWR_TRY(emit_dangling(g, dang_rows, dang_seeds, top_n, s));
        RWR_TRY(copy_lists_back(g, K_all, top_n, ids, scores, counts, row_stride));
        g->stats.seeds_done += K_all;
        g->stats.total_wall_ms += now_ms() - t_begin;
        return RWR_OK;
    }
    const int G = resolve_G(g, K);
    int TG = 1;
    RWR_TRY(ensure_workspace(g, G, K, &TG));
    const int ntiles = (int)cdiv((size_t)K, (size_t)G);
    std::vector<int32_t> slot_k, slot_seed;
    RWR_TRY(upload_seed_slots(g, seeds, K, G, &slot_k, &slot_seed));
    if (any_dangling) {   // slots map to positions in the live list: translate to the caller's batch positions
        for (auto &v : slot_k) if (v >= 0) v = live_rows[v];
        RWR_HIP(hipMemcpy(g->d_slot_k.p, slot_k.data(), slot_k.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    }

    // ranking inside the last step (rank_plan.h): the step runs over the first head_rows rows of tail_rows[0] only
    const bool select_path = top_n <= rank_select_max_k() && !rank_knobs().sort;
    const int32_t head_rows = fused_head_rows(g->n_items, g->vf != 0, top_n, select_path, rank_knobs());

    Profile prof(g);
    for (int t0 = 0; t0 < ntiles; t0 += TG) {
        const int tg = (ntiles - t0 < TG) ? (ntiles - t0) : TG;
        const int32_t *dseeds = g->d_seeds.p + (size_t)t0 * G;
        double *Xf = nullptr;
        hipEvent_t i0; RWR_TRY(prof.record(i0, s));
        int64_t dense_steps = 0;
        SplitLast split;
        split.head = head_rows;
        RWR_TRY(iterate_group(g, G, tg, dseeds, g->d_evoff.p + (size_t)t0 * G, slot_seed.data() + (size_t)t0 * G, d, n_iter,
                              prof, &Xf, &dense_steps, &split));
        RWR_TRY(prof.end(prof.iter, i0, s));
        int32_t real = 0;
        for (size_t q = (size_t)t0 * G; q < (size_t)(t0 + tg) * G; ++q) real += slot_k[q] >= 0;
        g->stats.spmm_seed_steps += (int64_t)real * n_iter;
        g->stats.spmm_dense_seed_steps += (int64_t)real * dense_steps;
        hipEvent_t a; RWR_TRY(prof.record(a, s));
        launch_exclude(g, G, tg, Xf, dseeds, s);
        RWR_HIP(hipGetLastError());
        const int32_t *slot_k_g = g->d_slot_k.p + (size_t)t0 * G;
        bool ranked = false;
        if (split.taken) RWR_TRY(rank_group_fused(g, G, tg, slot_k_g, dseeds, top_n, Xf, split, prof, s, &ranked));
        if (!ranked) RWR_TRY(rank_group(g, G, tg, slot_k_g, dseeds, top_n, Xf, s));
        RWR_TRY(prof.end(prof.rank, a, s));
    }
    if (any_dangling) RWR_TRY(emit_dangling(g, dang_rows, dang_seeds, top_n, s));
    RWR_TRY(copy_lists_back(g, K_all, top_n, ids, scores, counts, row_stride));
    RWR_HIP(hipStreamSynchronize(g->stream2));
    if (prof.on) RWR_TRY(chain_scan_collect(g, s));
    RWR_TRY(prof.fold(g));
    g->stats.tile_seeds = G;
    g->stats.tile_group = TG;
    g->stats.seeds_done += K_all;
    g->stats.total_wall_ms += now_ms() - t_begin;
    return RWR_OK;
}

}  // namespace rwr
