// The driver of rwr_eval_graphs: many ego-network-sized graphs built, walked and evaluated in chunks of 256 -- one build launch
// (graphs_build_multi, build_small.hip), one call launch (recommend_small_multi, small.hip) and one evaluation launch
// (eval_ranked_multi, rank.hip) per chunk --, the graphs these paths cannot take one by one through the public single-graph calls.
#include <algorithm>
#include <new>
#include <vector>
#include <stdlib.h>

#include "handle.h"

namespace rwr {

int32_t eval_graphs(int32_t count, const rwr_graph_desc *graphs, const int32_t *seeds, float d, int32_t n_iter,
                    const int64_t *test_ptr, const int64_t *test_ids, const rwr_opts *opts, int64_t *n_hits,
                    double *sum_precision, int64_t *list_len)
{
    static const char *const who = "rwr_eval_graphs";
#ifdef RWR_EXPERIMENTS
    const double t_enter = now_ms();
    double t_kit = 0, t_loop = 0;
#endif
    // a graph that the one-launch paths cannot take goes through the public single-graph calls
    auto one_by_one = [&](int32_t i) -> int32_t {
        const rwr_graph_desc &D = graphs[i];
        rwr_graph *g1 = nullptr;
        int32_t rc = rwr_graph_create(D.n_nodes, D.node_id, D.node_type, D.rowptr, D.dst, D.etype, D.w, opts, &g1);
        if (rc == RWR_OK)
            rc = rwr_recommend_eval(g1, seeds[i], d, n_iter, test_ids ? test_ids + test_ptr[i] : nullptr, test_ptr[i + 1] - test_ptr[i],
                                    n_hits + i, sum_precision + i, list_len ? list_len + i : nullptr);
        if (rc != RWR_OK) {
            char msg[600];
            snprintf(msg, sizeof(msg), "%s", rwr_last_error());
            set_error("graph %d of the batch: %s", i, msg);
        }
        if (g1) (void)rwr_graph_destroy(g1);
        return rc;
    };
    std::vector<int32_t> fast, slow;
    const bool d_ok = (double)d >= 0.0 && (double)d <= 1.0;
    for (int32_t i = 0; i < count; ++i) {
        const rwr_graph_desc &D = graphs[i];
        (d_ok && graph_fits_small_build(D.n_nodes, D.rowptr[D.n_nodes]) ? fast : slow).push_back(i);
    }
    if (!fast.empty()) {
        // the batch's stream comes from the handle pool (rwr_graph_create's); every graph of the batch works on it
        const int ndev = usable_devices();
        if (ndev <= 0) { set_error("no usable HIP device (librwr has no CPU fallback)"); return RWR_E_NO_DEVICE; }
        rwr_opts o{};
        RWR_TRY(resolve_opts(who, opts, ndev, false, &o));
        DeviceGuard dev_guard(o.device);
        if (dev_guard.rc != RWR_OK) return dev_guard.rc;
        RWR_TRY(check_gfx950(o.device));
        HandleKit kit;                       // (a full set, as rwr_graph_create makes one, so that the pool keeps it afterwards)
        RWR_TRY(kit_acquire(o.device, &kit));
        multi_pins_acquire();
        // Every pinned set starts at sizes the usual batch (tens of ego networks) never outgrows: growing a buffer is a
        // hipHostFree + hipHostMalloc -- milliseconds each, the first a device synchronisation --, and which set a call
        // gets changes from call to call, so sets sized by their first batch would keep growing for many calls when ten
        // threads with batches of different sizes share them.
        {
            static const size_t floor_bytes[5] = {(size_t)16 << 20, (size_t)256 << 10, (size_t)256 << 10, (size_t)1 << 20, (size_t)64 << 10};
            int32_t prc = RWR_OK;
            void *unused = nullptr;
            for (int sl = 0; sl < 5 && prc == RWR_OK; ++sl) prc = multi_pinned(sl, floor_bytes[sl], &unused);
            if (prc != RWR_OK) {
                multi_pins_release();
                kit_give(kit);
                return prc;
            }
        }
#ifdef RWR_EXPERIMENTS
        t_kit = now_ms();
        static const bool mt_on = [] { const char *e = getenv("RWR_X_MULTI_TIMING"); return e && atoi(e) != 0; }();
        double q0 = 0, q1 = 0, q2 = 0, q3 = 0;
#endif
        constexpr int32_t CHUNK = 256;                     // graphs per launch (a workgroup each)
        std::vector<rwr_graph *> gs;
        DevBuf<uint8_t> args_keep;                         // the call launch's argument table
        // a chunk's device buffers go back to the pool (nothing else is owned): only ever with kit.stream idle
        auto drop = [&]() {
            args_keep.release();
            for (rwr_graph *g : gs) delete g;
            gs.clear();
        };
        auto chunk = [&](size_t c0) -> int32_t {
            const int32_t nc = (int32_t)std::min<size_t>(CHUNK, fast.size() - c0);
            std::vector<rwr_graph_desc> descs((size_t)nc);
            gs.reserve((size_t)nc);
            for (int32_t q = 0; q < nc; ++q) {
                const int32_t i = fast[c0 + q];
                descs[q] = graphs[i];
                rwr_graph *g = new (std::nothrow) rwr_graph();
                if (!g) { set_error("out of host memory"); return RWR_E_NOMEM; }
                g->opts = o;
                g->device = o.device;
                g->n = graphs[i].n_nodes;
                g->nnz_raw = graphs[i].rowptr[graphs[i].n_nodes];
                g->stream = kit.stream;
                g->stats.struct_size = sizeof(rwr_stats);
                gs.push_back(g);
            }
            RWR_TRY(graphs_build_multi(gs.data(), nc, descs.data(), fast.data() + c0, kit.stream));
#ifdef RWR_EXPERIMENTS
            q1 = now_ms();
#endif
            // the one-launch call takes the graphs that pass its own limits (items, links, the seed's in-list)
            std::vector<rwr_graph *> run;
            std::vector<int32_t> run_seed, run_at;
            for (int32_t q = 0; q < nc; ++q) {
                const int32_t i = fast[c0 + q];
                rwr_graph *g = gs[q];
                if (g->n_items == 0) continue;             // (no candidates: hits 0, empty list)
                if (g->nonneg && small_path_ok(g) && small_path_seed_ok(g, seeds[i])) {
                    run.push_back(g);
                    run_seed.push_back(seeds[i]);
                    run_at.push_back(i);
                } else {
                    slow.push_back(i);
                }
            }
            if (run.empty()) return RWR_OK;
            const int32_t nr = (int32_t)run.size();
            // (args_keep lives until eval_ranked_multi has synchronised the stream)
            RWR_TRY(recommend_small_multi(run.data(), run_seed.data(), nr, (double)d, n_iter, kit.stream, args_keep));
#ifdef RWR_EXPERIMENTS
            q2 = now_ms();
#endif
            // HashSet<long> semantics per test set (Experiment.cs:124): sorted, duplicates dropped
            std::vector<int64_t> ts, tp((size_t)nr + 1, 0), hits((size_t)nr), lens((size_t)nr);
            std::vector<double> sums((size_t)nr);
            for (int32_t q = 0; q < nr; ++q) {
                const int32_t i = run_at[q];
                const size_t at = ts.size();
                if (test_ptr[i + 1] > test_ptr[i]) ts.insert(ts.end(), test_ids + test_ptr[i], test_ids + test_ptr[i + 1]);
                std::sort(ts.begin() + (long)at, ts.end());
                ts.erase(std::unique(ts.begin() + (long)at, ts.end()), ts.end());
                tp[(size_t)q + 1] = (int64_t)ts.size();
            }
            RWR_TRY(eval_ranked_multi(run.data(), nr, tp.data(), ts.data(), hits.data(), sums.data(), lens.data(), kit.stream));
            for (int32_t q = 0; q < nr; ++q) {
                const int32_t i = run_at[q];
                n_hits[i] = hits[q];
                sum_precision[i] = sums[q];
                if (list_len) list_len[i] = lens[q];
            }
            return RWR_OK;
        };
        int32_t rc = RWR_OK;
        for (size_t c0 = 0; c0 < fast.size() && rc == RWR_OK; c0 += CHUNK) {
#ifdef RWR_EXPERIMENTS
            q0 = now_ms();
            q1 = q2 = 0;
#endif
            rc = no_throw(who, [&] { return chunk(c0); });
            // a chunk that ran through ended in a synchronisation (the build's, or the evaluation's after the call launch); one
            // that failed may have work in flight, and nothing may be when the tables are released
            if (rc != RWR_OK) (void)hipStreamSynchronize(kit.stream);
#ifdef RWR_EXPERIMENTS
            q3 = now_ms();
#endif
            drop();
#ifdef RWR_EXPERIMENTS
            if (mt_on) fprintf(stderr, "[multi] %d graphs: build %.0f us, call enqueue %.0f, evaluation (incl. wait) %.0f, release %.0f\n",
                               (int32_t)std::min<size_t>(CHUNK, fast.size() - c0), 1e3 * (q1 - q0), 1e3 * (q2 - q1), 1e3 * (q3 - q2), 1e3 * (now_ms() - q3));
#endif
        }
#ifdef RWR_EXPERIMENTS
        t_loop = now_ms();
#endif
        (void)hipStreamSynchronize(kit.stream);
        multi_pins_release();
        kit_give(kit);
#ifdef RWR_EXPERIMENTS
        if (mt_on) fprintf(stderr, "[multi call] entry->kit %.0f us, chunks %.0f, tail %.0f\n", 1e3 * (t_kit - t_enter), 1e3 * (t_loop - t_kit),
                           1e3 * (now_ms() - t_loop));
#endif
        if (rc != RWR_OK) return rc;
    }
    std::sort(slow.begin(), slow.end());
    for (int32_t i : slow) RWR_TRY(one_by_one(i));
    return RWR_OK;
}

}  // namespace rwr
