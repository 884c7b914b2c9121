// K Models with caller-set restart vectors in one call (rwr_model_run_restart_batch): the cross product of
// restart.hip (one vector per call) and model.hip's batch of personalised Models (K seeds per call).
//
// Vector k sits in one slot (tile, lane) of the rank matrices X[tile][n][G].  One step of a tile group is
//   main stream    the link-only SpMM at G lanes: every row of every column receives its in-links in list order -- all a row
//                  outside the column's support receives (restart.hip: its restart addends are rr * 0);
//   second stream  k_restart_fold_cols: one in-order chain per (vector, support row) pair of the group, all in one launch,
//                  into a side buffer;
//   main stream    after the join, k_restart_scatter_cols puts the folded rows over the link-only values.
// Threshold modes sum |rank - nextRank| per column with the exact G-wide scan and stop each vector at its own step, as
// model_run_batch does for seeds; the finished columns leave through k_extract_cols and one D2H per row (GroupColumns).
//
// The SpMM runs the weighted kernels (ensure_in_w, as restart.hip): the step lasts as long as its chains, which the SpMM
// runs beside, so the value-free form's smaller matrix stream would shorten nothing (measured).
//
// rwr_recommend_restart_batch, rwr_recommend_restart_eval_batch (3.15) and rwr_recommend_restart_typed_batch
// (3.17) and rwr_recommend_restart_typed_positions_batch (3.19) are the same driver -- slot dealing, pair upload, step loop,
// statistics -- with another end of a tile group: after step T every vector's exclusion set is marked in X and the group is
// ranked or evaluated where it lies, so K x top_n entries, K records or the test ids' positions leave the device in place of
// K x n.  A RankedEnd (ranked_end.h) says which candidates, which exclusion and
// which destination, and does that work; the entries below only fill it in.  A call without one is the full-vector entry.
#include <algorithm>
#include <cstring>

#include "iterate.h"
#include "ranked_end.h"
#include "seed_row.h"

namespace rwr {

// Outside the batched domain: rwr_model_run_restart per vector, on the dense vector and the constructor's rank.  rk: each
// row goes back to the device as a tile of one lane -- vector k its own tile group of one slot -- for the same exclusion and
// ranking as a batched group's
static int32_t run_vector_by_vector(rwr_graph *g, int32_t K, const int64_t *sup_ptr, const int32_t *sup_idx, const double *sup_val,
                                    const int32_t *start, double d, int32_t run_mode, double value, double *rank_out,
                                    int64_t *iters_out, RankedEnd *rk, const char *who)
{
    const int32_t n = g->n;
    hipStream_t s = g->stream;
    std::vector<double> v((size_t)n), x((size_t)n), row(rk ? (size_t)n : 0);
    Profile prof(g);
    if (rk) {
        std::vector<int32_t> slot_k((size_t)K);
        for (int32_t k = 0; k < K; ++k) slot_k[(size_t)k] = k;
        RWR_TRY(g->d_slot_k.ensure((size_t)K));
        RWR_HIP(hipMemcpyAsync(g->d_slot_k.p, slot_k.data(), (size_t)K * sizeof(int32_t), hipMemcpyHostToDevice, s));
        RWR_TRY(rk->prepare(g, K, slot_k, 1, s));
        RWR_HIP(hipStreamSynchronize(s));
    }
    for (int32_t k = 0; k < K; ++k) {
        std::fill(v.begin(), v.end(), 0.0);
        for (int64_t q = sup_ptr[k]; q < sup_ptr[k + 1]; ++q) v[sup_idx[q]] = sup_val[q];
        const int32_t st = start ? start[k] : -1;
        std::fill(x.begin(), x.end(), st < 0 ? 1.0 : 0.0);         // Model.cs:25 / :44
        if (st >= 0) x[st] = (double)n;
        const int32_t rc = model_run_restart(g, v.data(), x.data(), d, run_mode, value, rk ? row.data() : rank_out + (size_t)k * n,
                                             iters_out ? iters_out + k : nullptr);
        if (rc != RWR_OK) {
            char msg[400];
            snprintf(msg, sizeof(msg), "%s", rwr_last_error());
            set_error("%s: vector %d: %s", who, k, msg);
            return rc;
        }
        if (rk) {
            RWR_TRY(g->X.ensure((size_t)n));
            RWR_HIP(hipMemcpyAsync(g->X.p, row.data(), sizeof(double) * (size_t)n, hipMemcpyHostToDevice, s));
            RWR_TRY(rk->finish_group(g, 1, 1, k, (size_t)k, g->X.p, prof, s));
            RWR_HIP(hipStreamSynchronize(s));                   // (the next vector's run reuses row and X)
            RWR_TRY(prof.fold(g));
        }
    }
    return RWR_OK;
}

// rk == nullptr: rwr_model_run_restart_batch, the finished columns leave as rows of rank_out.  Otherwise
// rwr_recommend_restart_batch (run_mode = RWR_RUN_ITERATIONS; a nonneg graph, d in [0, 1] and values >= 0 are api.hip's check):
// the finished groups are ranked on the device and the lists copied back once, after the last group
static int32_t restart_batch_body(rwr_graph *g, int32_t K, const int64_t *sup_ptr, const int32_t *sup_idx,
                                  const double *sup_val, const int32_t *start, double d, int32_t run_mode,
                                  double value, double *rank_out, int64_t *iters_out, RankedEnd *rk, const char *who)
{
    const double t_begin = now_ms();
    const int32_t n = g->n;
    // the non-zero entries of every vector (-0.0 counts as zero), and the batch-wide sign of the values
    std::vector<int64_t> nzp((size_t)K + 1, 0);
    bool v_nonneg = true, wide = false;
    for (int32_t k = 0; k < K; ++k) {
        int64_t c = 0;
        for (int64_t q = sup_ptr[k]; q < sup_ptr[k + 1]; ++q) {
            c += sup_val[q] != 0.0;
            v_nonneg = v_nonneg && sup_val[q] >= 0.0;
        }
        nzp[(size_t)k + 1] = nzp[k] + c;
        wide = wide || c > RWR_RESTART_EXACT_MAX;
    }
    // one vector, a vector of the tolerance class, or a graph / damping factor outside the domain of the batched kernels
    // (model_run_batch's policy): rwr_model_run_restart per vector, which the contract is equality with
    if (K == 1 || wide || !g->nonneg || !(d >= 0.0 && d <= 1.0)) {
        RWR_TRY(run_vector_by_vector(g, K, sup_ptr, sup_idx, sup_val, start, d, run_mode, value, rank_out, iters_out, rk, who));
        if (rk) {
            RWR_TRY(rk->copy_back(g, K));
            g->stats.seeds_done += K;
        }
        g->stats.total_wall_ms += now_ms() - t_begin;
        return RWR_OK;
    }
    const RunEnd end(run_mode, value, n);
    const double c1 = 1 - d;                                   // Model.cs:84
    const int G = resolve_G(g, K);
    int TG = 1;
    // + cs_diff: differences, then staging of the extracted columns (the ranked end needs neither)
    RWR_TRY(ensure_workspace(g, G, K, &TG, rk ? 0 : 1));
    const int ntiles = (int)cdiv((size_t)K, (size_t)G);
    const size_t slots = (size_t)ntiles * G;
    // vectors dealt to tile slots round-robin over the tiles (as upload_seed_slots deals seeds): slot_k = batch position, -1 =
    // padding; st = the slot's start node (-2 = padding: a zero column without support)
    std::vector<int32_t> slot_k(slots, -1), st(slots, -2), no_seed(slots, -1);
    for (int32_t k = 0; k < K; ++k) {
        const size_t slot = (size_t)(k % ntiles) * G + (size_t)(k / ntiles);
        slot_k[slot] = k;
        st[slot] = start ? start[k] : -1;
    }
    // the (vector, support row) pairs in slot order, pq relative to the slot's tile group; group gi's pairs are [gp[gi], gp[gi + 1])
    const int ngroups = (int)cdiv((size_t)ntiles, (size_t)TG);
    std::vector<int64_t> gp((size_t)ngroups + 1, 0);
    std::vector<int32_t> pq, pr;
    std::vector<double> pv;
    pq.reserve((size_t)nzp[K]); pr.reserve((size_t)nzp[K]); pv.reserve((size_t)nzp[K]);
    for (size_t slot = 0; slot < slots; ++slot) {
        const int grp = (int)(slot / G) / TG;
        const int32_t k = slot_k[slot];
        if (k >= 0)
            for (int64_t q = sup_ptr[k]; q < sup_ptr[k + 1]; ++q)
                if (sup_val[q] != 0.0) {
                    pq.push_back((int32_t)(slot - (size_t)grp * TG * G));
                    pr.push_back(sup_idx[q]);
                    pv.push_back(sup_val[q]);
                }
        gp[(size_t)grp + 1] = (int64_t)pq.size();
    }
    for (int gi = 1; gi <= ngroups; ++gi) gp[gi] = std::max(gp[gi], gp[gi - 1]);
    const size_t npairs_all = pq.size();

    hipStream_t s = g->stream, s2 = g->stream2;
    DevBuf<int32_t> d_pq, d_pr, d_st;
    DevBuf<double> d_pv, d_fold;
    StreamsIdle idle{g};
    RWR_TRY(ensure_in_w(g));                                    // the link-only SpMM runs the weighted kernels
    RWR_TRY(g->d_seeds.ensure(slots));
    RWR_TRY(g->d_evoff.ensure(slots + 1));
    RWR_TRY(g->d_evterm.ensure(1));
    RWR_TRY(g->d_part.ensure(MODEL_RED_PARTS + 8));
    RWR_TRY(g->cs_sums.ensure((size_t)TG * G));
    RWR_TRY(g->mb_row.ensure((size_t)TG * G));
    RWR_TRY(d_st.alloc(slots));
    RWR_HIP(hipMemcpyAsync(g->d_seeds.p, no_seed.data(), slots * sizeof(int32_t), hipMemcpyHostToDevice, s));
    RWR_HIP(hipMemsetAsync(g->d_evoff.p, 0, (slots + 1) * sizeof(int64_t), s));
    RWR_HIP(hipMemcpyAsync(d_st.p, st.data(), slots * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (npairs_all > 0) {
        RWR_TRY(d_pq.alloc(npairs_all));
        RWR_TRY(d_pr.alloc(npairs_all));
        RWR_TRY(d_pv.alloc(npairs_all));
        RWR_TRY(d_fold.alloc(npairs_all));
        RWR_HIP(hipMemcpyAsync(d_pq.p, pq.data(), npairs_all * sizeof(int32_t), hipMemcpyHostToDevice, s));
        RWR_HIP(hipMemcpyAsync(d_pr.p, pr.data(), npairs_all * sizeof(int32_t), hipMemcpyHostToDevice, s));
        RWR_HIP(hipMemcpyAsync(d_pv.p, pv.data(), npairs_all * sizeof(double), hipMemcpyHostToDevice, s));
    }
    if (rk) {                                                   // (d_slot_k: the ranking's output-row table and liveness array)
        RWR_TRY(g->d_slot_k.ensure(slots));
        RWR_HIP(hipMemcpyAsync(g->d_slot_k.p, slot_k.data(), slots * sizeof(int32_t), hipMemcpyHostToDevice, s));
        RWR_TRY(rk->prepare(g, K, slot_k, (size_t)TG * G, s));
    }
    RWR_HIP(hipStreamSynchronize(s));                           // (the host vectors above are pageable)

    Profile prof(g);                                            // (column extraction counts as ranking time)
    int32_t stuck = -1;                                         // threshold modes: smallest k that did not converge
    for (int t0 = 0, grp = 0; t0 < ntiles; t0 += TG, ++grp) {
        const int tg = (ntiles - t0 < TG) ? (ntiles - t0) : TG;
        const size_t q0 = (size_t)t0 * G;
        const int32_t npairs = (int32_t)(gp[(size_t)grp + 1] - gp[grp]);
        const int32_t *gq = d_pq.p + gp[grp], *gr = d_pr.p + gp[grp];
        const double *gv = d_pv.p + gp[grp];
        double *gf = d_fold.p + gp[grp];
        GroupColumns cols(g, G, tg, slot_k.data() + q0, g->d_evoff.p + q0, end, rank_out, iters_out, prof);
        double *X = g->X.p, *Y = g->Y.p;
        launch_restart_init_cols(g, G, tg, d_st.p + q0, X, s);  // Model ctor (Model.cs:25 / :44)
        RWR_HIP(hipGetLastError());
        if (!end.by_count) RWR_TRY(chain_scan_sum_cols_prepare(g, G, tg, s));
        SpmmArgs sp;                                            // link-only: no seed row, every row, no bitmaps, no row lists
        sp.seeds = g->d_seeds.p + q0, sp.c1 = c1;
        // restart.hip's rule, batch-wide: the constructors' ranks are >= 0 and stay so while every restart value is
        sp.hub_scan = v_nonneg;
        int64_t steps = 0;
        for (;;) {
            if (rk && steps == end.T) {                         // every column ends here and stays on the device
                RWR_TRY(rk->finish_group(g, G, tg, grp, q0, X, prof, s));
                break;
            }
            if (cols.ends.due(steps)) {
                RWR_TRY(cols.emit(steps, X));
                if (cols.ends.done()) break;
            }
            if (steps == end.T) {                               // RWR_MAX_ITERS steps made: the later groups still decide the smallest k
                if (stuck < 0 || cols.ends.stuck() < stuck) stuck = cols.ends.stuck();
                break;
            }
            hipEvent_t i0; RWR_TRY(prof.record(i0, s));
            if (npairs > 0) {                                   // the support rows' chains beside the SpMM
                RWR_HIP(hipEventRecord(g->ev_fork, s));
                RWR_HIP(hipStreamWaitEvent(s2, g->ev_fork, 0));
                hipEvent_t c0; RWR_TRY(prof.record(c0, s2));
                launch_restart_fold_cols(g, G, npairs, gq, gr, gv, X, c1, gf, s2);
                RWR_HIP(hipGetLastError());
                RWR_TRY(prof.end(prof.chain, c0, s2));
                RWR_HIP(hipEventRecord(g->ev_join, s2));
            }
            hipEvent_t a; RWR_TRY(prof.record(a, s));
            sp.X = X, sp.Y = Y;
            launch_spmm(g, G, tg, sp, s);
            RWR_TRY(prof.end(prof.spmm, a, s));
            if (prof.on) prof.dense.push_back(1);
            if (npairs > 0) {
                RWR_HIP(hipStreamWaitEvent(s, g->ev_join, 0));
                launch_restart_scatter_cols(g, G, npairs, gq, gr, gf, Y, s);
            }
            RWR_HIP(hipGetLastError());
            std::swap(X, Y);                                    // Model.updateRanks (Model.cs:103-108)
            ++steps;
            g->stats.spmm_launches += 1;
            g->stats.spmm_dense_launches += 1;
            g->stats.chain_launches += npairs > 0;
            RWR_TRY(end.by_count ? prof.end(prof.iter, i0, s) : cols.measure(i0, Y, X));
        }
        cols.count(steps, steps);
    }
    if (rk) {                                                   // one copy-back of K x top_n entries, as recommend_batch's (or of K records)
        RWR_TRY(rk->copy_back(g, K));
        g->stats.seeds_done += K;
    }
    RWR_TRY(finish_model_batch(g, prof, G, TG, t_begin));
    if (stuck >= 0) {
        set_error("%s: vector %d: no convergence within %lld iterations (RWR_MAX_ITERS)", who, stuck,
                  (long long)end.max_iters);
        return RWR_E_UNSUPPORTED;
    }
    return RWR_OK;
}

int32_t model_run_restart_batch(rwr_graph *g, int32_t K, const int64_t *sup_ptr, const int32_t *sup_idx, const double *sup_val,
                                const int32_t *start, double d, int32_t run_mode, double value, double *rank_out,
                                int64_t *iters_out)
{
    static const char *const who = "rwr_model_run_restart_batch";
    return no_throw(who, [&] {
        return restart_batch_body(g, K, sup_ptr, sup_idx, sup_val, start, d, run_mode, value, rank_out, iters_out, nullptr, who);
    });
}

// the ranked entries: T steps, then the end they describe
static int32_t restart_ranked(rwr_graph *g, int32_t K, const int64_t *sup_ptr, const int32_t *sup_idx, const double *sup_val,
                              const int32_t *start, double d, int32_t n_iter, RankedEnd &end, int32_t cand_type = -1)
{
    StreamsIdle idle{g};                                        // (declared after end: ranked_end.h)
    return no_throw(end.who, [&] {
        // (a type's list is fetched before the workspace is sized from what is free)
        if (cand_type >= 0) RWR_TRY(cand_rows_get(g, cand_type, &end.rows, &end.nrows));
        return restart_batch_body(g, K, sup_ptr, sup_idx, sup_val, start, d, RWR_RUN_ITERATIONS, (double)n_iter, nullptr, nullptr,
                                  &end, end.who);
    });
}

int32_t recommend_restart_batch(rwr_graph *g, int32_t K, const int64_t *sup_ptr, const int32_t *sup_idx, const double *sup_val,
                                const int32_t *start, const int64_t *set_ptr, const int32_t *set_idx, double d, int32_t n_iter,
                                int32_t top_n, int64_t *ids, double *scores, int32_t *counts)
{
    RankedEnd end;                                              // the ITEM rows, the sets' raw LIKE links, lists
    end.who = "rwr_recommend_restart_batch";
    end.set_ptr = set_ptr, end.set_idx = set_idx, end.mask = 1u << RWR_EDGE_LIKE;
    end.top_n = top_n, end.ids = ids, end.scores = scores, end.counts = counts;
    return restart_ranked(g, K, sup_ptr, sup_idx, sup_val, start, d, n_iter, end);
}

int32_t recommend_restart_typed_batch(rwr_graph *g, int32_t K, const int64_t *sup_ptr, const int32_t *sup_idx,
                                      const double *sup_val, const int32_t *start, const int64_t *set_ptr, const int32_t *set_idx,
                                      double d, int32_t n_iter, int32_t top_n, int32_t cand_type, uint32_t excl_edge_mask,
                                      int32_t exclude_members, int64_t *ids, double *scores, int32_t *counts)
{
    RankedEnd end;                                              // the rows of a type, the links of the mask and the members, lists
    end.who = "rwr_recommend_restart_typed_batch";
    end.set_ptr = set_ptr, end.set_idx = set_idx, end.mask = excl_edge_mask, end.members = exclude_members != 0;
    end.top_n = top_n, end.ids = ids, end.scores = scores, end.counts = counts;
    return restart_ranked(g, K, sup_ptr, sup_idx, sup_val, start, d, n_iter, end, cand_type);
}

int32_t recommend_restart_eval_batch(rwr_graph *g, int32_t K, const int64_t *sup_ptr, const int32_t *sup_idx, const double *sup_val,
                                     const int32_t *start, const int64_t *set_ptr, const int32_t *set_idx, double d, int32_t n_iter,
                                     int32_t top_n, const int64_t *test_ptr, const int64_t *test_ids, int64_t *n_hits,
                                     double *sum_precision, int64_t *list_len)
{
    EvalEnd ev;
    ev.test_ptr = test_ptr, ev.test_ids = test_ids, ev.top_n = top_n;
    ev.n_hits = n_hits, ev.sum_precision = sum_precision, ev.list_len = list_len;
    RankedEnd end;                                              // the ITEM rows, the sets' raw LIKE links, records
    end.who = "rwr_recommend_restart_eval_batch";
    end.set_ptr = set_ptr, end.set_idx = set_idx, end.mask = 1u << RWR_EDGE_LIKE;
    end.ev = &ev;
    return restart_ranked(g, K, sup_ptr, sup_idx, sup_val, start, d, n_iter, end);
}

int32_t recommend_restart_typed_positions_batch(rwr_graph *g, int32_t K, const int64_t *sup_ptr, const int32_t *sup_idx,
                                                const double *sup_val, const int32_t *start, const int64_t *set_ptr,
                                                const int32_t *set_idx, double d, int32_t n_iter, int32_t cand_type,
                                                uint32_t excl_edge_mask, int32_t exclude_members, const int64_t *test_ptr,
                                                const int64_t *test_ids, int64_t *pos_out, double *score_out, int64_t *list_len)
{
    PosEnd pe;
    pe.ev.test_ptr = test_ptr, pe.ev.test_ids = test_ids;
    pe.pos_out = pos_out, pe.score_out = score_out, pe.list_len = list_len;
    RankedEnd end;                                              // the rows of a type, the links of the mask and the members, positions
    end.who = "rwr_recommend_restart_typed_positions_batch";
    end.set_ptr = set_ptr, end.set_idx = set_idx, end.mask = excl_edge_mask, end.members = exclude_members != 0;
    end.pos = &pe;
    return restart_ranked(g, K, sup_ptr, sup_idx, sup_val, start, d, n_iter, end, cand_type);
}

}  // namespace rwr
