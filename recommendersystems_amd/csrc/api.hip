// C-ABI entry points of librwr (include/rwr.h): the thread's error string, every argument check, and one call each into the
// drivers.  No CPU fallback anywhere: without a usable gfx950 device every compute entry fails with RWR_E_NO_DEVICE.
#include <stdarg.h>
#include <algorithm>
#include <cmath>
#include <vector>
#include <string.h>

#include "audience.h"
#include "audience_plan.h"
#include "eval_plan.h"
#include "exclude_plan.h"
#include "handle.h"
#include "long_plan.h"
#include "rank.h"
#include "typed_call.h"

namespace rwr {

static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// The device work of an entry point, after its argument checks: a poisoned handle is refused, the graph's device is current
// while `body` runs (DeviceGuard), and no C++ exception leaves (no_throw).  `who` names the entry in no_throw's messages.
template <class F>
static int32_t bound(const char *who, rwr_graph *g, F &&body)
{
    if (g->poisoned) {
        set_error("this graph handle was invalidated by a failed rebuild (rwr_graph_update_links / rwr_graph_append_links / rwr_graph_append_nodes / rwr_graph_remove_links / rwr_graph_remove_nodes); destroy it");
        return RWR_E_INVALID;
    }
    DeviceGuard dev_guard(g->device);
    if (dev_guard.rc != RWR_OK) return dev_guard.rc;
    return no_throw(who, body);
}

// ... of an edit that fills NEW buffers and hands them to the handle (append.hip, remove.hip, node_remove.hip): before the swap
// the handle still holds the old lists and everything derived from them, so a failure there leaves it usable; a failure after
// it (`body` has set *swapped) leaves derived arrays that no longer match the new lists, and the handle is poisoned.
template <class F>
static int32_t bound_edit(const char *who, rwr_graph *g, F &&body)
{
    bool swapped = false;
    const int32_t rc = bound(who, g, [&] { return body(&swapped); });
    if (rc != RWR_OK && swapped) g->poisoned = 1;
    return rc;
}

// The arrays of one graph as rwr_graph_create and rwr_eval_graphs take them.  The messages open with "<who>:" (at < 0) or
// "<who>: graph <at>:" and call the node count n_name.
static int32_t check_graph_arrays(const char *who, int32_t at, const char *n_name, int32_t n, const int64_t *node_id,
                                  const uint8_t *node_type, const int64_t *rowptr, const int32_t *dst, const uint8_t *etype,
                                  const double *w)
{
    char pre[96];
    auto prefix = [&] {
        if (at < 0) snprintf(pre, sizeof(pre), "%s:", who);
        else snprintf(pre, sizeof(pre), "%s: graph %d:", who, at);
        return pre;
    };
    if (n <= 0 || !node_id || !node_type || !rowptr) {
        set_error("%s %s must be > 0 and node_id/node_type/rowptr non-NULL", prefix(), n_name);
        return RWR_E_INVALID;
    }
    if (rowptr[0] != 0) { set_error("%s rowptr[0] must be 0", prefix()); return RWR_E_INVALID; }
    for (int32_t i = 0; i < n; ++i)
        if (rowptr[i + 1] < rowptr[i]) {
            set_error("%s rowptr decreases at node %d", prefix(), i);
            return RWR_E_INVALID;
        }
    if (rowptr[n] > 0 && (!dst || !etype || !w)) {
        set_error("%s dst/etype/w must be non-NULL when there are links", prefix());
        return RWR_E_INVALID;
    }
    return RWR_OK;
}

// the run modes of Model.run (rwr.h); `who` names the entry in the message
static int32_t check_run_mode(const char *who, int32_t run_mode)
{
    if (run_mode == RWR_RUN_ITERATIONS || run_mode == RWR_RUN_THRESHOLD || run_mode == RWR_RUN_DEFAULT_THRESHOLD) return RWR_OK;
    set_error("%s: unknown run_mode %d", who, run_mode);
    return RWR_E_INVALID;
}

// The K restart vectors of a batch (CSR) and their start nodes, as both batched restart entries take them: the pointer array,
// then per vector its start, its indices and values, and that no index appears twice.  `who` names the entry in the message.
static int32_t check_restart_vectors(const char *who, int32_t n, int32_t K, const int64_t *sup_ptr, const int32_t *sup_idx,
                                     const double *sup_val, const int32_t *start)
{
    if (sup_ptr[0] != 0) { set_error("%s: sup_ptr[0] = %lld, not 0", who, (long long)sup_ptr[0]); return RWR_E_INVALID; }
    for (int32_t k = 0; k < K; ++k)
        if (sup_ptr[k + 1] < sup_ptr[k]) {
            set_error("%s: sup_ptr decreases at batch position %d", who, k);
            return RWR_E_INVALID;
        }
    if (sup_ptr[K] > 0 && (!sup_idx || !sup_val)) { set_error("%s: NULL sup_idx or sup_val", who); return RWR_E_INVALID; }
    try {
        std::vector<int32_t> sorted;
        for (int32_t k = 0; k < K; ++k) {
            if (start && (start[k] < -1 || start[k] >= n)) {
                set_error("%s: start %d (batch position %d) is outside [-1, %d)", who, start[k], k, n);
                return RWR_E_RANGE;
            }
            for (int64_t q = sup_ptr[k]; q < sup_ptr[k + 1]; ++q) {
                if (sup_idx[q] < 0 || sup_idx[q] >= n) {
                    set_error("%s: index %d (batch position %d) is outside [0, %d)", who, sup_idx[q], k, n);
                    return RWR_E_RANGE;
                }
                if (!std::isfinite(sup_val[q])) {
                    set_error("%s: restart[%d] = %g (batch position %d) is not finite (rr * 0 would be NaN in every row)", who,
                              sup_idx[q], sup_val[q], k);
                    return RWR_E_UNSUPPORTED;
                }
            }
            sorted.assign(sup_idx + sup_ptr[k], sup_idx + sup_ptr[k + 1]);
            std::sort(sorted.begin(), sorted.end());
            const auto dup = std::adjacent_find(sorted.begin(), sorted.end());
            if (dup != sorted.end()) {
                set_error("%s: index %d appears twice in vector %d", who, *dup, k);
                return RWR_E_INVALID;
            }
        }
    } catch (const std::bad_alloc &) {
        set_error("%s: host allocation failed", who);
        return RWR_E_NOMEM;
    }
    return RWR_OK;
}

// The vectors and exclusion sets of a ranked restart batch, as rwr_recommend_restart_batch and rwr_recommend_restart_eval_batch
// take them: what check_restart_vectors reports, then the first negative value, then exclude_check's verdict
static int32_t check_ranked_vectors(const char *who, int32_t n, int32_t K, const int64_t *sup_ptr, const int32_t *sup_idx,
                                    const double *sup_val, const int32_t *start, const int64_t *excl_ptr, const int32_t *excl_idx)
{
    RWR_TRY(check_restart_vectors(who, n, K, sup_ptr, sup_idx, sup_val, start));
    // the domain of the Recommendation entries: the exclusion marker (-1) and the ranking keys assume scores >= 0
    for (int32_t k = 0; k < K; ++k)
        for (int64_t q = sup_ptr[k]; q < sup_ptr[k + 1]; ++q)
            if (sup_val[q] < 0.0) {
                set_error("%s: restart[%d] = %g (batch position %d) is negative: ranks could go negative; "
                          "rwr_model_run_restart_batch runs signed vectors", who, sup_idx[q], sup_val[q], k);
                return RWR_E_UNSUPPORTED;
            }
    if (excl_ptr) {
        const ExcludeCheck c = exclude_check(n, K, excl_ptr, excl_idx);
        switch (c.verdict) {
            case EXCLUDE_OK: break;
            case EXCLUDE_BAD_PTR0:
                set_error("%s: excl_ptr[0] = %lld, not 0", who, (long long)excl_ptr[0]);
                return RWR_E_INVALID;
            case EXCLUDE_PTR_DECREASES:
                set_error("%s: excl_ptr decreases at batch position %d", who, c.bad_k);
                return RWR_E_INVALID;
            case EXCLUDE_NULL_IDX:
                set_error("%s: NULL excl_idx", who);
                return RWR_E_INVALID;
            case EXCLUDE_BAD_INDEX:
                set_error("%s: exclusion index %d (batch position %d) is outside [0, %d)", who, c.bad_index, c.bad_k, n);
                return RWR_E_RANGE;
        }
    }
    return RWR_OK;
}

// a refusal worded on the host (typed_call.h) into the thread's error string; RWR_OK passes through
static int32_t report(const CallStatus &st)
{
    if (st.status != RWR_OK) set_error("%s", st.text);
    return st.status;
}

// ... and the graph and damping factor of the Recommendation entries: the exclusion marker (-1) and the ranking keys assume
// scores >= 0.  model_entry: the entry that runs what this one refuses
static int32_t check_ranked_domain(const char *who, const rwr_graph *g, double d, const char *model_entry)
{
    if (!g->nonneg) {
        set_error("%s: Recommendation needs non-negative finite link weights and positive row sums; %s accepts such graphs", who,
                  model_entry);
        return RWR_E_UNSUPPORTED;
    }
    if (!(d >= 0.0 && d <= 1.0)) {
        set_error("%s: Recommendation needs a damping factor in [0, 1] (got %g); %s accepts any value", who, d, model_entry);
        return RWR_E_UNSUPPORTED;
    }
    return RWR_OK;
}

// What every seed-driven typed entry does with the call it has filled in: typed_call.h's ladder, the no-op, the refusal, the
// domain, and the one driver
static int32_t typed_entry(const char *who, rwr_graph *g, const TypedCall &call, float d, int32_t n_iter)
{
    g_err[0] = 0;
    const int32_t n = g ? g->n : 0;
    const CallCheck c = typed_call_check(call, g != nullptr, n, rank_select_max_k());
    if (c.verdict == CALL_NOOP) return RWR_OK;
    RWR_TRY(report(call_status(who, c, call, n, rank_select_max_k())));
    RWR_TRY(check_ranked_domain(who, g, (double)d, "rwr_model_run_batch"));
    if (n_iter < 0) n_iter = 0;   // Model.run(int): a non-positive count runs no iteration (Model.cs:69)
    // Recommender.cs:14,16 -> Model.cs:33: the float is widened to double
    return bound(who, g, [&] { return typed_body(g, call, (double)d, n_iter, who); });
}

}  // namespace rwr

using namespace rwr;

extern "C" {

const char *rwr_version(void) { return RWR_VERSION_STRING " (gfx950, hip)"; }

int32_t rwr_device_count(void) { return usable_devices(); }

const char *rwr_last_error(void) { return g_err; }

int32_t rwr_graph_create(int32_t n, const int64_t *node_id, const uint8_t *node_type, const int64_t *rowptr,
                         const int32_t *dst, const uint8_t *etype, const double *w, const rwr_opts *opts,
                         rwr_graph **out)
{
    g_err[0] = 0;
    if (!out) { set_error("rwr_graph_create: out is NULL"); return RWR_E_INVALID; }
    *out = nullptr;
    RWR_TRY(check_graph_arrays("rwr_graph_create", -1, "n", n, node_id, node_type, rowptr, dst, etype, w));
    return no_throw("rwr_graph_create", [&] { return graph_open(n, node_id, node_type, rowptr, dst, etype, w, opts, out); });
}

int32_t rwr_graph_update_links(rwr_graph *g, int64_t count, const int64_t *link_index, const uint8_t *etype,
                               const double *w)
{
    g_err[0] = 0;
    if (!g) { set_error("rwr_graph_update_links: graph is NULL"); return RWR_E_INVALID; }
    if (count < 0 || (count > 0 && !link_index)) {
        set_error("rwr_graph_update_links: count must be >= 0 and link_index non-NULL when count > 0");
        return RWR_E_INVALID;
    }
    bool began = false;       // (a handle whose device could not be bound was not touched: it stays as it is)
    const int32_t rc = bound("rwr_graph_update_links", g, [&] { began = true; return graph_update_links(g, count, link_index, etype, w); });
    // a failure after the raw lists were patched leaves derived arrays that no longer match them
    if (began && rc != RWR_OK && rc != RWR_E_RANGE && rc != RWR_E_INVALID) g->poisoned = 1;
    return rc;
}

int32_t rwr_graph_append_links(rwr_graph *g, int64_t count, const int32_t *src, const int32_t *dst, const uint8_t *etype,
                               const double *w, int64_t *new_index_out)
{
    g_err[0] = 0;
    if (!g) { set_error("rwr_graph_append_links: graph is NULL"); return RWR_E_INVALID; }
    if (count < 0 || (count > 0 && (!src || !dst || !etype || !w))) {
        set_error("rwr_graph_append_links: count must be >= 0 and src/dst/etype/w non-NULL when count > 0");
        return RWR_E_INVALID;
    }
    return bound_edit("rwr_graph_append_links", g, [&](bool *swapped) {
        return graph_append(g, "rwr_graph_append_links", 0, nullptr, nullptr, count, src, dst, etype, w, new_index_out, swapped);
    });
}

int32_t rwr_graph_append_nodes(rwr_graph *g, int32_t n_new, const int64_t *node_id, const uint8_t *node_type, int64_t count,
                               const int32_t *src, const int32_t *dst, const uint8_t *etype, const double *w,
                               int64_t *new_index_out)
{
    g_err[0] = 0;
    if (!g) { set_error("rwr_graph_append_nodes: graph is NULL"); return RWR_E_INVALID; }
    if (n_new < 0 || (n_new > 0 && (!node_id || !node_type))) {
        set_error("rwr_graph_append_nodes: n_new must be >= 0 and node_id/node_type non-NULL when n_new > 0");
        return RWR_E_INVALID;
    }
    if (count < 0 || (count > 0 && (!src || !dst || !etype || !w))) {
        set_error("rwr_graph_append_nodes: count must be >= 0 and src/dst/etype/w non-NULL when count > 0");
        return RWR_E_INVALID;
    }
    // (node types are taken as rwr_graph_create takes them: unchecked, anything but ITEM is no candidate)
    return bound_edit("rwr_graph_append_nodes", g, [&](bool *swapped) {
        return graph_append(g, "rwr_graph_append_nodes", n_new, node_id, node_type, count, src, dst, etype, w, new_index_out, swapped);
    });
}

int32_t rwr_graph_remove_links(rwr_graph *g, int64_t count, const int64_t *link_index)
{
    g_err[0] = 0;
    if (!g) { set_error("rwr_graph_remove_links: graph is NULL"); return RWR_E_INVALID; }
    if (count < 0 || (count > 0 && !link_index)) {
        set_error("rwr_graph_remove_links: count must be >= 0 and link_index non-NULL when count > 0");
        return RWR_E_INVALID;
    }
    return bound_edit("rwr_graph_remove_links", g, [&](bool *swapped) { return graph_remove(g, count, link_index, swapped); });
}

int32_t rwr_graph_remove_nodes(rwr_graph *g, int32_t count, const int32_t *node_index, int32_t *new_node_index_out,
                               int64_t *new_link_index_out, int64_t *links_removed_out)
{
    g_err[0] = 0;
    if (!g) { set_error("rwr_graph_remove_nodes: graph is NULL"); return RWR_E_INVALID; }
    if (count < 0 || (count > 0 && !node_index)) {
        set_error("rwr_graph_remove_nodes: count must be >= 0 and node_index non-NULL when count > 0");
        return RWR_E_INVALID;
    }
    return bound_edit("rwr_graph_remove_nodes", g, [&](bool *swapped) {
        return graph_remove_nodes(g, count, node_index, new_node_index_out, new_link_index_out, links_removed_out, swapped);
    });
}

int32_t rwr_graph_destroy(rwr_graph *g)
{
    if (!g) return RWR_OK;
    graph_close(g);           // (throws nothing: handle.hip)
    return RWR_OK;
}

int32_t rwr_graph_size(const rwr_graph *g, int32_t *n, int64_t *nnz_raw, int64_t *nnz_explicit)
{
    if (!g) { set_error("rwr_graph_size: graph is NULL"); return RWR_E_INVALID; }
    if (n) *n = g->n;
    if (nnz_raw) *nnz_raw = g->nnz_raw;
    if (nnz_explicit) *nnz_explicit = g->nnz;
    return RWR_OK;
}

int32_t rwr_graph_get_normalized(rwr_graph *g, double *w_out, uint8_t *dangling_out)
{
    g_err[0] = 0;
    if (!g) { set_error("rwr_graph_get_normalized: graph is NULL"); return RWR_E_INVALID; }
    return bound("rwr_graph_get_normalized", g, [&]() -> int32_t {
        if (w_out && g->nnz_raw > 0)
            RWR_HIP(hipMemcpy(w_out, g->w_norm_raw.p, sizeof(double) * (size_t)g->nnz_raw, hipMemcpyDeviceToHost));
        if (dangling_out) RWR_HIP(hipMemcpy(dangling_out, g->dangling.p, (size_t)g->n, hipMemcpyDeviceToHost));
        return RWR_OK;
    });
}

int32_t rwr_eval_graphs(int32_t count, const rwr_graph_desc *graphs, const int32_t *seeds, float d, int32_t n_iter,
                        const int64_t *test_ptr, const int64_t *test_ids, const rwr_opts *opts, int64_t *n_hits,
                        double *sum_precision, int64_t *list_len)
{
    g_err[0] = 0;
    if (count < 0 || (count > 0 && (!graphs || !seeds || !test_ptr || !n_hits || !sum_precision))) {
        set_error("rwr_eval_graphs: bad argument");
        return RWR_E_INVALID;
    }
    if (count == 0) return RWR_OK;
    if (n_iter < 0) n_iter = 0;
    for (int32_t i = 0; i < count; ++i) {
        const rwr_graph_desc &D = graphs[i];
        RWR_TRY(check_graph_arrays("rwr_eval_graphs", i, "n_nodes", D.n_nodes, D.node_id, D.node_type, D.rowptr, D.dst, D.etype, D.w));
        if (seeds[i] < 0 || seeds[i] >= D.n_nodes) { set_error("graph %d: seed %d is outside [0, %d)", i, seeds[i], D.n_nodes); return RWR_E_RANGE; }
        if (test_ptr[i + 1] < test_ptr[i] || test_ptr[i + 1] - test_ptr[i] > 0x7FFFFFFF) {
            set_error("rwr_eval_graphs: test_ptr must be non-decreasing (graph %d)", i);
            return RWR_E_INVALID;
        }
    }
    if (test_ptr[count] > test_ptr[0] && !test_ids) { set_error("rwr_eval_graphs: test_ids is NULL"); return RWR_E_INVALID; }
    for (int32_t i = 0; i < count; ++i) { n_hits[i] = 0; sum_precision[i] = 0.0; if (list_len) list_len[i] = 0; }
    return no_throw("rwr_eval_graphs",
                    [&] { return eval_graphs(count, graphs, seeds, d, n_iter, test_ptr, test_ids, opts, n_hits, sum_precision, list_len); });
}

int32_t rwr_recommend_batch(rwr_graph *g, const int32_t *seeds, int32_t K, float d, int32_t n_iter, int32_t top_n,
                            int64_t *ids, double *scores, int32_t *counts)
{
    g_err[0] = 0;
    if (!g || !seeds || !ids || !scores || !counts) { set_error("rwr_recommend_batch: NULL argument"); return RWR_E_INVALID; }
    if (K <= 0) { set_error("rwr_recommend_batch: K must be >= 1"); return RWR_E_INVALID; }
    if (top_n < 1) { set_error("rwr_recommend_batch: top_n must be >= 1"); return RWR_E_INVALID; }
    if (n_iter < 0) n_iter = 0;   // Model.run(int): a non-positive count runs no iteration (Model.cs:69)
    // Recommender.cs:14,16 -> Model.cs:33: the float is widened to double
    return bound("rwr_recommend_batch", g, [&] { return recommend_batch(g, seeds, K, (double)d, n_iter, top_n, ids, scores, counts, top_n); });
}

int32_t rwr_recommend_typed_batch(rwr_graph *g, const int32_t *seeds, int32_t K, float d, int32_t n_iter, int32_t top_n,
                                  int32_t cand_type, uint32_t excl_edge_mask, int32_t exclude_self, int64_t *ids, double *scores,
                                  int32_t *counts)
{
    TypedCall c;
    c.seeds = seeds, c.K = K, c.cand_type = cand_type, c.excl_edge_mask = excl_edge_mask, c.exclude_self = exclude_self;
    c.top_n = top_n, c.ids = ids, c.scores = scores, c.counts = counts;
    c.top_n_hint = " (rwr_recommend_typed_eval_batch evaluates whole lists of a node type)";
    return typed_entry("rwr_recommend_typed_batch", g, c, d, n_iter);
}

int32_t rwr_recommend_typed_eval_batch(rwr_graph *g, const int32_t *seeds, int32_t K, float d, int32_t n_iter, int32_t top_n,
                                       int32_t cand_type, uint32_t excl_edge_mask, int32_t exclude_self, const int64_t *test_ptr,
                                       const int64_t *test_ids, int64_t *n_hits, double *sum_precision, int64_t *list_len)
{
    TypedCall c;
    c.seeds = seeds, c.K = K, c.cand_type = cand_type, c.excl_edge_mask = excl_edge_mask, c.exclude_self = exclude_self;
    c.dest = CALL_EVAL, c.top_n = top_n;                         // (no list is written: top_n has no bound here)
    c.test_ptr = test_ptr, c.test_ids = test_ids, c.n_hits = n_hits, c.sum_precision = sum_precision, c.list_len = list_len;
    return typed_entry("rwr_recommend_typed_eval_batch", g, c, d, n_iter);
}

int32_t rwr_recommend_typed_positions_batch(rwr_graph *g, const int32_t *seeds, int32_t K, float d, int32_t n_iter, int32_t cand_type,
                                            uint32_t excl_edge_mask, int32_t exclude_self, const int64_t *test_ptr,
                                            const int64_t *test_ids, int64_t *pos_out, double *score_out, int64_t *list_len)
{
    TypedCall c;
    c.seeds = seeds, c.K = K, c.cand_type = cand_type, c.excl_edge_mask = excl_edge_mask, c.exclude_self = exclude_self;
    c.dest = CALL_POSITIONS;
    c.test_ptr = test_ptr, c.test_ids = test_ids, c.pos_out = pos_out, c.score_out = score_out, c.list_len = list_len;
    return typed_entry("rwr_recommend_typed_positions_batch", g, c, d, n_iter);
}

int32_t rwr_recommend_filtered_batch(rwr_graph *g, const int32_t *seeds, int32_t K, float d, int32_t n_iter, int32_t top_n,
                                     int32_t cand_type, uint32_t excl_edge_mask, int32_t exclude_self, int64_t pool_count,
                                     const int32_t *pool_idx, const int64_t *deny_ptr, const int32_t *deny_idx, int64_t *ids,
                                     double *scores, int32_t *counts)
{
    TypedCall c;
    c.seeds = seeds, c.K = K, c.cand_type = cand_type, c.excl_edge_mask = excl_edge_mask, c.exclude_self = exclude_self;
    c.any_type = true, c.pool_count = pool_count, c.pool_idx = pool_idx, c.deny_ptr = deny_ptr, c.deny_idx = deny_idx;
    c.top_n = top_n, c.ids = ids, c.scores = scores, c.counts = counts;
    c.top_n_hint = " (rwr_recommend_filtered_positions_batch answers for whole lists)";
    return typed_entry("rwr_recommend_filtered_batch", g, c, d, n_iter);
}

int32_t rwr_recommend_filtered_positions_batch(rwr_graph *g, const int32_t *seeds, int32_t K, float d, int32_t n_iter,
                                               int32_t cand_type, uint32_t excl_edge_mask, int32_t exclude_self, int64_t pool_count,
                                               const int32_t *pool_idx, const int64_t *deny_ptr, const int32_t *deny_idx,
                                               const int64_t *test_ptr, const int64_t *test_ids, int64_t *pos_out, double *score_out,
                                               int64_t *list_len)
{
    TypedCall c;
    c.seeds = seeds, c.K = K, c.cand_type = cand_type, c.excl_edge_mask = excl_edge_mask, c.exclude_self = exclude_self;
    c.any_type = true, c.pool_count = pool_count, c.pool_idx = pool_idx, c.deny_ptr = deny_ptr, c.deny_idx = deny_idx;
    c.dest = CALL_POSITIONS;
    c.test_ptr = test_ptr, c.test_ids = test_ids, c.pos_out = pos_out, c.score_out = score_out, c.list_len = list_len;
    return typed_entry("rwr_recommend_filtered_positions_batch", g, c, d, n_iter);
}

int32_t rwr_recommend_capped_batch(rwr_graph *g, const int32_t *seeds, int32_t K, float d, int32_t n_iter, int32_t top_n,
                                   int32_t cand_type, uint32_t excl_edge_mask, int32_t exclude_self, int64_t pool_count,
                                   const int32_t *pool_idx, const int64_t *deny_ptr, const int32_t *deny_idx, const int32_t *group_of,
                                   int32_t group_cap, int64_t *ids, double *scores, int32_t *counts)
{
    TypedCall c;
    c.seeds = seeds, c.K = K, c.cand_type = cand_type, c.excl_edge_mask = excl_edge_mask, c.exclude_self = exclude_self;
    c.any_type = true, c.pool_count = pool_count, c.pool_idx = pool_idx, c.deny_ptr = deny_ptr, c.deny_idx = deny_idx;
    c.group_of = group_of, c.group_cap = group_cap;
    c.top_n = top_n, c.ids = ids, c.scores = scores, c.counts = counts;
    c.top_n_hint = " (rwr_recommend_capped_positions_batch answers for whole lists)";
    return typed_entry("rwr_recommend_capped_batch", g, c, d, n_iter);
}

int32_t rwr_recommend_capped_positions_batch(rwr_graph *g, const int32_t *seeds, int32_t K, float d, int32_t n_iter,
                                             int32_t cand_type, uint32_t excl_edge_mask, int32_t exclude_self, int64_t pool_count,
                                             const int32_t *pool_idx, const int64_t *deny_ptr, const int32_t *deny_idx,
                                             const int32_t *group_of, int32_t group_cap, const int64_t *test_ptr,
                                             const int64_t *test_ids, int64_t *pos_out, double *score_out, int64_t *list_len)
{
    TypedCall c;
    c.seeds = seeds, c.K = K, c.cand_type = cand_type, c.excl_edge_mask = excl_edge_mask, c.exclude_self = exclude_self;
    c.any_type = true, c.pool_count = pool_count, c.pool_idx = pool_idx, c.deny_ptr = deny_ptr, c.deny_idx = deny_idx;
    c.group_of = group_of, c.group_cap = group_cap;
    c.dest = CALL_POSITIONS;
    c.test_ptr = test_ptr, c.test_ids = test_ids, c.pos_out = pos_out, c.score_out = score_out, c.list_len = list_len;
    return typed_entry("rwr_recommend_capped_positions_batch", g, c, d, n_iter);
}

int32_t rwr_recommend_explained_batch(rwr_graph *g, const int32_t *seeds, int32_t K, float d, int32_t n_iter, int32_t top_n,
                                      int32_t cand_type, uint32_t excl_edge_mask, int32_t exclude_self, int64_t pool_count,
                                      const int32_t *pool_idx, const int64_t *deny_ptr, const int32_t *deny_idx, const int32_t *group_of,
                                      int32_t group_cap, int32_t n_why, int64_t *ids, double *scores, int32_t *counts, int32_t *nodes,
                                      int32_t *why_src, double *why_term, int64_t *why_total)
{
    TypedCall c;
    c.seeds = seeds, c.K = K, c.cand_type = cand_type, c.excl_edge_mask = excl_edge_mask, c.exclude_self = exclude_self;
    c.any_type = true, c.pool_count = pool_count, c.pool_idx = pool_idx, c.deny_ptr = deny_ptr, c.deny_idx = deny_idx;
    c.group_of = group_of, c.group_cap = group_cap;
    c.top_n = top_n, c.ids = ids, c.scores = scores, c.counts = counts;
    c.n_why = n_why, c.nodes = nodes, c.why_src = why_src, c.why_term = why_term, c.why_total = why_total;
    return typed_entry("rwr_recommend_explained_batch", g, c, d, n_iter);
}

// The audience of K targets (audience.hip).  The refusals in rwr.h's order: the handle, audience_plan.h's ladder,
// the domain, and only then the no-op
int32_t rwr_recommend_audience_batch(rwr_graph *g, int32_t K, const int32_t *targets, float d, int32_t n_iter, int32_t cand_type,
                                     uint32_t etype_mask, int32_t exclude_self, int32_t top_n, int64_t *out_id, double *out_score,
                                     int32_t *out_node, int32_t *out_count)
{
    const char *who = "rwr_recommend_audience_batch";
    g_err[0] = 0;
    const int32_t n = g ? g->n : 0;
    if (g && g->poisoned) return bound(who, g, [] { return (int32_t)RWR_OK; });   // (bound words the refusal of such a handle)
    const AudCheck c = audience_check(g != nullptr, n, K, targets, n_iter, cand_type, etype_mask, top_n, out_id, out_score, out_count);
    switch (c.verdict) {
        case AUD_OK:
        case AUD_NOOP: break;
        case AUD_NULL_GRAPH: set_error("%s: NULL graph", who); return RWR_E_INVALID;
        case AUD_NEGATIVE_K: set_error("%s: negative K", who); return RWR_E_INVALID;
        case AUD_NULL_ARG: set_error("%s: NULL targets, out_id, out_score or out_count", who); return RWR_E_INVALID;
        case AUD_TARGET_RANGE:
            set_error("%s: target %d (batch position %d) is outside [0, %d)", who, c.bad_target, c.bad_k, n);
            return RWR_E_RANGE;
        case AUD_TOP_N_RANGE: set_error("%s: top_n %d is outside [1, %d]", who, top_n, (int)AUD_TOP_N_MAX); return RWR_E_RANGE;
        case AUD_NEGATIVE_ITER:
            set_error("%s: n_iter %d is negative (a fixed number of steps only: the threshold modes have no reverse counterpart)", who, n_iter);
            return RWR_E_INVALID;
        case AUD_BAD_CAND_TYPE: set_error("%s: cand_type %d is outside [-1, 255]", who, cand_type); return RWR_E_INVALID;
        case AUD_BAD_MASK:
            set_error("%s: etype_mask 0x%x has a bit beyond the %u edge types", who, etype_mask, TYPED_EDGE_TYPES);
            return RWR_E_INVALID;
    }
    RWR_TRY(check_ranked_domain(who, g, (double)d, "rwr_model_run_batch"));
    if (K == 0) return RWR_OK;
    // the same body as the set entries: set k = {targets[k]}, weight 1.0, no pool, no deny lists
    // Recommender.cs:14,16 -> Model.cs:33: the float is widened to double
    return bound(who, g, [&] {
        std::vector<int64_t> set_ptr((size_t)K + 1);
        for (int32_t k = 0; k <= K; ++k) set_ptr[(size_t)k] = k;
        AudCall call;
        call.K = K, call.set_ptr = set_ptr.data(), call.set_idx = targets, call.n_iter = n_iter, call.cand_type = cand_type;
        call.etype_mask = etype_mask, call.exclude_members = exclude_self;
        call.top_n = top_n, call.out_id = out_id, call.out_score = out_score, call.out_node = out_node, call.out_count = out_count;
        return audience_body(g, call, (double)d, who);
    });
}

// The audiences of K weighted target sets (audience.hip), for both destinations.  The refusals in rwr.h's
// order: the handle, audience_set_plan.h's ladder -- which also words every refusal --, the domain, and only then the no-op
static int32_t audience_set_entry(const char *who, rwr_graph *g, const AudCall &call, float d)
{
    g_err[0] = 0;
    const int32_t n = g ? g->n : 0;
    if (g && g->poisoned) return bound(who, g, [] { return (int32_t)RWR_OK; });   // (bound words the refusal of such a handle)
    const AudStatus st = audience_set_status(who, audience_set_check(call, g != nullptr, n), call, n);
    if (st.status != RWR_OK) { set_error("%s", st.text); return st.status; }
    RWR_TRY(check_ranked_domain(who, g, (double)d, "rwr_model_run_batch"));
    if (call.K == 0) return RWR_OK;
    return bound(who, g, [&] { return audience_body(g, call, (double)d, who); });
}

int32_t rwr_recommend_audience_set_batch(rwr_graph *g, int32_t K, const int64_t *set_ptr, const int32_t *set_idx, const double *set_w,
                                         float d, int32_t n_iter, int32_t cand_type, uint32_t etype_mask, int32_t exclude_members,
                                         int32_t n_pool, const int32_t *pool_idx, const int64_t *deny_ptr, const int32_t *deny_idx,
                                         int32_t top_n, int64_t *out_id, double *out_score, int32_t *out_node, int32_t *out_count)
{
    AudCall c;
    c.K = K, c.set_ptr = set_ptr, c.set_idx = set_idx, c.set_w = set_w, c.n_iter = n_iter, c.cand_type = cand_type;
    c.etype_mask = etype_mask, c.exclude_members = exclude_members, c.n_pool = n_pool, c.pool_idx = pool_idx;
    c.deny_ptr = deny_ptr, c.deny_idx = deny_idx;
    c.top_n = top_n, c.out_id = out_id, c.out_score = out_score, c.out_node = out_node, c.out_count = out_count;
    return audience_set_entry("rwr_recommend_audience_set_batch", g, c, d);
}

int32_t rwr_recommend_audience_set_positions_batch(rwr_graph *g, int32_t K, const int64_t *set_ptr, const int32_t *set_idx,
                                                   const double *set_w, float d, int32_t n_iter, int32_t cand_type,
                                                   uint32_t etype_mask, int32_t exclude_members, int32_t n_pool,
                                                   const int32_t *pool_idx, const int64_t *deny_ptr, const int32_t *deny_idx,
                                                   const int64_t *test_ptr, const int64_t *test_ids, int64_t *out_pos,
                                                   double *out_score, int64_t *out_len)
{
    AudCall c;
    c.K = K, c.set_ptr = set_ptr, c.set_idx = set_idx, c.set_w = set_w, c.n_iter = n_iter, c.cand_type = cand_type;
    c.etype_mask = etype_mask, c.exclude_members = exclude_members, c.n_pool = n_pool, c.pool_idx = pool_idx;
    c.deny_ptr = deny_ptr, c.deny_idx = deny_idx;
    c.dest = AUD_POSITIONS;
    c.test_ptr = test_ptr, c.test_ids = test_ids, c.out_pos = out_pos, c.out_score = out_score, c.out_len = out_len;
    return audience_set_entry("rwr_recommend_audience_set_positions_batch", g, c, d);
}

// Lists of up to RWR_LONG_TOP_N_MAX entries (long_list.hip): the explained entry's call without reasons and the
// audience set entry's call, each with long_plan.h's top_n limit in its ladder; the drivers name the long destination from
// top_n alone
int32_t rwr_recommend_long_batch(rwr_graph *g, const int32_t *seeds, int32_t K, float d, int32_t n_iter, int32_t top_n,
                                 int32_t cand_type, uint32_t excl_edge_mask, int32_t exclude_self, int64_t pool_count,
                                 const int32_t *pool_idx, const int64_t *deny_ptr, const int32_t *deny_idx, const int32_t *group_of,
                                 int32_t group_cap, int64_t *ids, double *scores, int32_t *counts, int32_t *nodes)
{
    TypedCall c;
    c.seeds = seeds, c.K = K, c.cand_type = cand_type, c.excl_edge_mask = excl_edge_mask, c.exclude_self = exclude_self;
    c.pool_count = pool_count, c.pool_idx = pool_idx, c.deny_ptr = deny_ptr, c.deny_idx = deny_idx;
    c.group_of = group_of, c.group_cap = group_cap;
    c.top_n = top_n, c.ids = ids, c.scores = scores, c.counts = counts, c.nodes = nodes;
    long_call_fill(c);
    return typed_entry("rwr_recommend_long_batch", g, c, d, n_iter);
}

int32_t rwr_recommend_audience_set_long_batch(rwr_graph *g, int32_t K, const int64_t *set_ptr, const int32_t *set_idx, const double *set_w,
                                              float d, int32_t n_iter, int32_t cand_type, uint32_t etype_mask, int32_t exclude_members,
                                              int32_t n_pool, const int32_t *pool_idx, const int64_t *deny_ptr, const int32_t *deny_idx,
                                              int32_t top_n, int64_t *out_id, double *out_score, int32_t *out_node, int32_t *out_count)
{
    AudCall c;
    c.K = K, c.set_ptr = set_ptr, c.set_idx = set_idx, c.set_w = set_w, c.n_iter = n_iter, c.cand_type = cand_type;
    c.etype_mask = etype_mask, c.exclude_members = exclude_members, c.n_pool = n_pool, c.pool_idx = pool_idx;
    c.deny_ptr = deny_ptr, c.deny_idx = deny_idx;
    c.top_n = top_n, c.out_id = out_id, c.out_score = out_score, c.out_node = out_node, c.out_count = out_count;
    long_aud_fill(c);
    return audience_set_entry("rwr_recommend_audience_set_long_batch", g, c, d);
}

int32_t rwr_recommend(rwr_graph *g, int32_t seed, float d, int32_t n_iter, int32_t top_n, int64_t *out_id,
                      double *out_score, int64_t *inout_count)
{
    g_err[0] = 0;
    if (!g || !inout_count) { set_error("rwr_recommend: NULL argument"); return RWR_E_INVALID; }
    if (seed < 0 || seed >= g->n) { set_error("seed %d is outside [0, %d)", seed, g->n); return RWR_E_RANGE; }
    if (n_iter < 0) n_iter = 0;
    return bound("rwr_recommend", g, [&]() -> int32_t {
        // Recommender.cs:42-51: topN <= 0 never truncates
        int64_t width = (top_n > 0 && top_n < g->n_items) ? top_n : g->n_items;
        if (width == 0) { *inout_count = 0; return RWR_OK; }
        if (width > 0x7FFFFFFF) { set_error("rwr_recommend: list too long"); return RWR_E_UNSUPPORTED; }
        int32_t cnt = 0;
        if (width <= small_pin_words() && out_id && out_score && *inout_count >= width &&
            !(small_path_ok(g) && small_path_seed_ok(g, seed))) {
            // a short list (top-N of a large graph): count, ids and scores come back into the handle's pinned buffer behind ONE
            // synchronisation (waiting for the count first and copying then cost a second host round trip: ~90 us of a 1.6 ms call)
            RWR_TRY(small_pin_ensure(g));
            int64_t *pid = const_cast<int64_t *>(small_pin_ids(g));
            double *psc = const_cast<double *>(small_pin_scores(g));
            g->sm_pin_count = -1;
            RWR_TRY(recommend_batch(g, &seed, 1, (double)d, n_iter, (int32_t)width, pid, psc, &cnt, width));
            memcpy(out_id, pid, sizeof(int64_t) * (size_t)cnt);
            memcpy(out_score, psc, sizeof(double) * (size_t)cnt);
            *inout_count = cnt;
            return RWR_OK;
        }
        // the ranked list stays on the device until its length is known, then goes straight into the caller's arrays
        // (no host staging copy: the full list of a 5 M-item graph is 80 MB)
        g->sm_pin_count = -1;
        RWR_TRY(recommend_batch(g, &seed, 1, (double)d, n_iter, (int32_t)width, nullptr, nullptr, &cnt, width));
        if (*inout_count < cnt || ((!out_id || !out_score) && cnt > 0)) {
            set_error("rwr_recommend: output holds %lld entries, %d needed", (long long)*inout_count, cnt);
            *inout_count = cnt;
            return RWR_E_CAPACITY;
        }
        if (cnt > 0 && g->sm_pin_count == cnt) {
            // ego-network-sized graph (small.hip): the kernel wrote the list into pinned host memory
            memcpy(out_id, small_pin_ids(g), sizeof(int64_t) * (size_t)cnt);
            memcpy(out_score, small_pin_scores(g), sizeof(double) * (size_t)cnt);
        } else if (cnt > 0) {
            RWR_HIP(hipMemcpyAsync(out_id, g->d_out_id.p, sizeof(int64_t) * (size_t)cnt, hipMemcpyDeviceToHost, g->stream));
            RWR_HIP(hipMemcpyAsync(out_score, g->d_out_score.p, sizeof(double) * (size_t)cnt, hipMemcpyDeviceToHost, g->stream));
            RWR_HIP(hipStreamSynchronize(g->stream));
        }
        *inout_count = cnt;
        return RWR_OK;
    });
}

int32_t rwr_recommend_eval(rwr_graph *g, int32_t seed, float d, int32_t n_iter, const int64_t *test_ids,
                           int64_t n_test, int64_t *n_hits, double *sum_precision, int64_t *list_len)
{
    g_err[0] = 0;
    if (!g || !n_hits || !sum_precision || (n_test > 0 && !test_ids) || n_test < 0) {
        set_error("rwr_recommend_eval: bad argument");
        return RWR_E_INVALID;
    }
    if (seed < 0 || seed >= g->n) { set_error("seed %d is outside [0, %d)", seed, g->n); return RWR_E_RANGE; }
    if (n_test > 0x7FFFFFFF) { set_error("rwr_recommend_eval: test set too large"); return RWR_E_UNSUPPORTED; }
    if (n_iter < 0) n_iter = 0;
    return bound("rwr_recommend_eval", g, [&]() -> int32_t {
        *n_hits = 0;
        *sum_precision = 0.0;
        if (list_len) *list_len = 0;
        const int32_t width = g->n_items;
        if (width == 0) return RWR_OK;
        int32_t cnt = 0;
        RWR_TRY(recommend_batch(g, &seed, 1, (double)d, n_iter, width, nullptr, nullptr, &cnt, width));
        std::vector<int64_t> ts(test_ids, test_ids + n_test);
        std::sort(ts.begin(), ts.end());
        ts.erase(std::unique(ts.begin(), ts.end()), ts.end());     // HashSet<long>
        RWR_TRY(eval_ranked(g, cnt, ts.data(), (int64_t)ts.size(), n_hits, sum_precision));
        if (list_len) *list_len = cnt;
        return RWR_OK;
    });
}

int32_t rwr_recommend_eval_batch(rwr_graph *g, const int32_t *seeds, int32_t K, float d, int32_t n_iter,
                                 const int64_t *test_ptr, const int64_t *test_ids, int64_t *n_hits, double *sum_precision,
                                 int64_t *list_len)
{
    g_err[0] = 0;
    if (!g || !seeds || K < 0 || !test_ptr || !n_hits || !sum_precision) {
        set_error("rwr_recommend_eval_batch: bad argument");
        return RWR_E_INVALID;
    }
    for (int32_t k = 0; k < K; ++k) {
        if (seeds[k] < 0 || seeds[k] >= g->n) { set_error("seed %d (batch position %d) is outside [0, %d)", seeds[k], k, g->n); return RWR_E_RANGE; }
        if (test_ptr[k + 1] < test_ptr[k] || test_ptr[k + 1] - test_ptr[k] > 0x7FFFFFFF) {
            set_error("rwr_recommend_eval_batch: test_ptr must be non-decreasing (position %d)", k);
            return RWR_E_INVALID;
        }
    }
    if (K > 0 && test_ptr[K] > test_ptr[0] && !test_ids) { set_error("rwr_recommend_eval_batch: test_ids is NULL"); return RWR_E_INVALID; }
    if (n_iter < 0) n_iter = 0;
    return bound("rwr_recommend_eval_batch", g, [&]() -> int32_t {
        for (int32_t k = 0; k < K; ++k) { n_hits[k] = 0; sum_precision[k] = 0.0; if (list_len) list_len[k] = 0; }
        const int32_t width = g->n_items;
        if (width == 0 || K == 0) return RWR_OK;
        // HashSet<long> semantics per test set (Experiment.cs:124): sorted, duplicates dropped; offsets rebuilt
        std::vector<int64_t> ts, tp((size_t)K + 1, 0);
        ts.reserve((size_t)(test_ptr[K] - test_ptr[0]));
        for (int32_t k = 0; k < K; ++k) {
            const size_t at = ts.size();
            ts.insert(ts.end(), test_ids + test_ptr[k], test_ids + test_ptr[k + 1]);
            std::sort(ts.begin() + at, ts.end());
            ts.erase(std::unique(ts.begin() + at, ts.end()), ts.end());
            tp[(size_t)k + 1] = (int64_t)ts.size();
        }
        // the full ranked lists stay on the device, `chunk` seeds at a time (16 bytes per candidate and seed)
        const int64_t per_seed = (int64_t)width * 16;
        int32_t chunk = (int32_t)std::max<int64_t>(1, std::min<int64_t>(K, (1ll << 30) / std::max<int64_t>(per_seed, 1)));
        std::vector<int32_t> cnt((size_t)K);
        for (int32_t k0 = 0; k0 < K; k0 += chunk) {
            const int32_t kc = std::min(chunk, K - k0);
            RWR_TRY(recommend_batch(g, seeds + k0, kc, (double)d, n_iter, width, nullptr, nullptr, cnt.data() + k0, width));
            std::vector<int64_t> tpc((size_t)kc + 1);
            for (int32_t q = 0; q <= kc; ++q) tpc[q] = tp[(size_t)k0 + q] - tp[k0];
            RWR_TRY(eval_ranked_batch(g, kc, width, tpc.data(), ts.data() + tp[k0], n_hits + k0, sum_precision + k0));
        }
        if (list_len) for (int32_t k = 0; k < K; ++k) list_len[k] = cnt[k];
        return RWR_OK;
    });
}

int32_t rwr_model_deliver(rwr_graph *g, int32_t seed, double d, const double *rank, double *next_rank)
{
    g_err[0] = 0;
    if (!g || !rank || !next_rank || rank == next_rank) { set_error("rwr_model_deliver: NULL or aliasing argument"); return RWR_E_INVALID; }
    return bound("rwr_model_deliver", g, [&] { return model_deliver(g, seed, d, rank, next_rank); });
}

int32_t rwr_model_run(rwr_graph *g, int32_t seed, double d, int32_t run_mode, double value, double *rank_out,
                      int64_t *iters_out)
{
    g_err[0] = 0;
    if (!g || !rank_out) { set_error("rwr_model_run: NULL argument"); return RWR_E_INVALID; }
    return bound("rwr_model_run", g, [&]() -> int32_t {
        RWR_TRY(check_run_mode("rwr_model_run", run_mode));
        return model_run(g, seed, d, run_mode, value, rank_out, iters_out);
    });
}

int32_t rwr_model_run_batch(rwr_graph *g, const int32_t *seeds, int32_t K, double d, int32_t run_mode, double value,
                            double *rank_out, int64_t *iters_out)
{
    g_err[0] = 0;
    if (!g || K < 0 || (K > 0 && (!seeds || !rank_out))) {
        set_error("rwr_model_run_batch: NULL argument or negative K");
        return RWR_E_INVALID;
    }
    RWR_TRY(check_run_mode("rwr_model_run_batch", run_mode));
    for (int32_t k = 0; k < K; ++k)
        if (seeds[k] < 0 || seeds[k] >= g->n) {   // (-1, the global model, stays on rwr_model_run)
            set_error("rwr_model_run_batch: seed %d (batch position %d) is outside [0, %d)", seeds[k], k, g->n);
            return RWR_E_RANGE;
        }
    if (K == 0) return RWR_OK;
    return bound("rwr_model_run_batch", g, [&] { return model_run_batch(g, seeds, K, d, run_mode, value, rank_out, iters_out); });
}

int32_t rwr_model_run_restart(rwr_graph *g, const double *restart, const double *rank_in, double d, int32_t run_mode,
                              double value, double *rank_out, int64_t *iters_out)
{
    g_err[0] = 0;
    if (!g || !restart || !rank_in || !rank_out) { set_error("rwr_model_run_restart: NULL argument"); return RWR_E_INVALID; }
    RWR_TRY(check_run_mode("rwr_model_run_restart", run_mode));
    return bound("rwr_model_run_restart", g, [&] { return model_run_restart(g, restart, rank_in, d, run_mode, value, rank_out, iters_out); });
}

int32_t rwr_model_run_restart_batch(rwr_graph *g, int32_t K, const int64_t *sup_ptr, const int32_t *sup_idx,
                                    const double *sup_val, const int32_t *start, double d, int32_t run_mode, double value,
                                    double *rank_out, int64_t *iters_out)
{
    static const char *const who = "rwr_model_run_restart_batch";
    g_err[0] = 0;
    if (!g) { set_error("%s: NULL graph", who); return RWR_E_INVALID; }
    if (K < 0) { set_error("%s: negative K", who); return RWR_E_INVALID; }
    if (K == 0) return RWR_OK;
    if (!sup_ptr || !rank_out) { set_error("%s: NULL sup_ptr or rank_out", who); return RWR_E_INVALID; }
    RWR_TRY(check_run_mode(who, run_mode));
    RWR_TRY(check_restart_vectors(who, g->n, K, sup_ptr, sup_idx, sup_val, start));
    return bound(who, g, [&] { return model_run_restart_batch(g, K, sup_ptr, sup_idx, sup_val, start, d, run_mode, value, rank_out, iters_out); });
}

int32_t rwr_recommend_restart_batch(rwr_graph *g, int32_t K, const int64_t *sup_ptr, const int32_t *sup_idx,
                                    const double *sup_val, const int32_t *start, const int64_t *excl_ptr,
                                    const int32_t *excl_idx, double d, int32_t n_iter, int32_t top_n, int64_t *ids,
                                    double *scores, int32_t *counts)
{
    static const char *const who = "rwr_recommend_restart_batch";
    g_err[0] = 0;
    if (!g) { set_error("%s: NULL graph", who); return RWR_E_INVALID; }
    if (K < 0) { set_error("%s: negative K", who); return RWR_E_INVALID; }
    if (K == 0) return RWR_OK;
    if (!sup_ptr || !ids || !scores || !counts) { set_error("%s: NULL sup_ptr, ids, scores or counts", who); return RWR_E_INVALID; }
    if (top_n < 1) { set_error("%s: top_n must be >= 1", who); return RWR_E_INVALID; }
    RWR_TRY(check_ranked_vectors(who, g->n, K, sup_ptr, sup_idx, sup_val, start, excl_ptr, excl_idx));
    RWR_TRY(check_ranked_domain(who, g, d, "rwr_model_run_restart_batch"));
    if (n_iter < 0) n_iter = 0;   // Model.run(int): a non-positive count runs no iteration (Model.cs:69)
    // excl_ptr == NULL: set k is the indices of vector k's support, whatever their values
    return bound(who, g, [&] {
        return recommend_restart_batch(g, K, sup_ptr, sup_idx, sup_val, start, excl_ptr ? excl_ptr : sup_ptr,
                                       excl_ptr ? excl_idx : sup_idx, d, n_iter, top_n, ids, scores, counts);
    });
}

int32_t rwr_recommend_restart_typed_batch(rwr_graph *g, int32_t K, const int64_t *sup_ptr, const int32_t *sup_idx,
                                          const double *sup_val, const int32_t *start, const int64_t *excl_ptr,
                                          const int32_t *excl_idx, double d, int32_t n_iter, int32_t top_n, int32_t cand_type,
                                          uint32_t excl_edge_mask, int32_t exclude_members, int64_t *ids, double *scores,
                                          int32_t *counts)
{
    static const char *const who = "rwr_recommend_restart_typed_batch";
    g_err[0] = 0;
    if (!g) { set_error("%s: NULL graph", who); return RWR_E_INVALID; }
    if (K < 0) { set_error("%s: negative K", who); return RWR_E_INVALID; }
    if (K == 0) return RWR_OK;
    if (!sup_ptr || !ids || !scores || !counts) { set_error("%s: NULL sup_ptr, ids, scores or counts", who); return RWR_E_INVALID; }
    TypedCall t;                                                 // (the graph, K and the pointers were looked at above)
    t.top_n = top_n, t.cand_type = cand_type, t.excl_edge_mask = excl_edge_mask;
    CallCheck c;
    c.verdict = restart_typed_check(top_n, rank_select_max_k(), cand_type, excl_edge_mask);
    RWR_TRY(report(call_status(who, c, t, g->n, rank_select_max_k())));
    RWR_TRY(check_ranked_vectors(who, g->n, K, sup_ptr, sup_idx, sup_val, start, excl_ptr, excl_idx));
    RWR_TRY(check_ranked_domain(who, g, d, "rwr_model_run_restart_batch"));
    if (n_iter < 0) n_iter = 0;   // Model.run(int): a non-positive count runs no iteration (Model.cs:69)
    // excl_ptr == NULL: set k is the indices of vector k's support, whatever their values
    return bound(who, g, [&] {
        return recommend_restart_typed_batch(g, K, sup_ptr, sup_idx, sup_val, start, excl_ptr ? excl_ptr : sup_ptr,
                                             excl_ptr ? excl_idx : sup_idx, d, n_iter, top_n, cand_type, excl_edge_mask,
                                             exclude_members, ids, scores, counts);
    });
}

int32_t rwr_recommend_restart_eval_batch(rwr_graph *g, int32_t K, const int64_t *sup_ptr, const int32_t *sup_idx,
                                         const double *sup_val, const int32_t *start, const int64_t *excl_ptr,
                                         const int32_t *excl_idx, double d, int32_t n_iter, int32_t top_n,
                                         const int64_t *test_ptr, const int64_t *test_ids, int64_t *n_hits,
                                         double *sum_precision, int64_t *list_len)
{
    static const char *const who = "rwr_recommend_restart_eval_batch";
    g_err[0] = 0;
    if (!g) { set_error("%s: NULL graph", who); return RWR_E_INVALID; }
    if (K < 0) { set_error("%s: negative K", who); return RWR_E_INVALID; }
    if (K == 0) return RWR_OK;
    if (!sup_ptr) { set_error("%s: NULL sup_ptr", who); return RWR_E_INVALID; }
    RWR_TRY(check_ranked_vectors(who, g->n, K, sup_ptr, sup_idx, sup_val, start, excl_ptr, excl_idx));
    RWR_TRY(report(eval_status(who, eval_check(K, test_ptr, test_ids, n_hits, sum_precision), test_ptr, "n_hits or sum_precision")));
    RWR_TRY(check_ranked_domain(who, g, d, "rwr_model_run_restart_batch"));
    if (n_iter < 0) n_iter = 0;   // Model.run(int): a non-positive count runs no iteration (Model.cs:69)
    return bound(who, g, [&] {
        return recommend_restart_eval_batch(g, K, sup_ptr, sup_idx, sup_val, start, excl_ptr ? excl_ptr : sup_ptr,
                                            excl_ptr ? excl_idx : sup_idx, d, n_iter, top_n, test_ptr, test_ids, n_hits,
                                            sum_precision, list_len);
    });
}

int32_t rwr_recommend_restart_typed_positions_batch(rwr_graph *g, int32_t K, const int64_t *sup_ptr, const int32_t *sup_idx,
                                                    const double *sup_val, const int32_t *start, const int64_t *excl_ptr,
                                                    const int32_t *excl_idx, double d, int32_t n_iter, int32_t cand_type,
                                                    uint32_t excl_edge_mask, int32_t exclude_members, const int64_t *test_ptr,
                                                    const int64_t *test_ids, int64_t *pos_out, double *score_out, int64_t *list_len)
{
    static const char *const who = "rwr_recommend_restart_typed_positions_batch";
    g_err[0] = 0;
    if (!g) { set_error("%s: NULL graph", who); return RWR_E_INVALID; }
    if (K < 0) { set_error("%s: negative K", who); return RWR_E_INVALID; }
    if (K == 0) return RWR_OK;
    if (!sup_ptr) { set_error("%s: NULL sup_ptr", who); return RWR_E_INVALID; }
    TypedCall t;                                                 // (no top_n here: the whole lists)
    t.cand_type = cand_type, t.excl_edge_mask = excl_edge_mask;
    CallCheck c;
    c.verdict = restart_typed_check(1, 1, cand_type, excl_edge_mask);
    RWR_TRY(report(call_status(who, c, t, g->n, rank_select_max_k())));
    RWR_TRY(check_ranked_vectors(who, g->n, K, sup_ptr, sup_idx, sup_val, start, excl_ptr, excl_idx));
    RWR_TRY(report(eval_status(who, eval_check(K, test_ptr, test_ids, pos_out, pos_out), test_ptr, "pos_out")));
    RWR_TRY(check_ranked_domain(who, g, d, "rwr_model_run_restart_batch"));
    if (n_iter < 0) n_iter = 0;   // Model.run(int): a non-positive count runs no iteration (Model.cs:69)
    // excl_ptr == NULL: set k is the indices of vector k's support, whatever their values
    return bound(who, g, [&] {
        return recommend_restart_typed_positions_batch(g, K, sup_ptr, sup_idx, sup_val, start, excl_ptr ? excl_ptr : sup_ptr,
                                                       excl_ptr ? excl_idx : sup_idx, d, n_iter, cand_type, excl_edge_mask,
                                                       exclude_members, test_ptr, test_ids, pos_out, score_out, list_len);
    });
}

int32_t rwr_model_deliver_restart(rwr_graph *g, const double *restart, double d, const double *rank, double *next_rank)
{
    g_err[0] = 0;
    if (!g || !restart || !rank || !next_rank) { set_error("rwr_model_deliver_restart: NULL argument"); return RWR_E_INVALID; }
    return bound("rwr_model_deliver_restart", g, [&] { return model_deliver_restart(g, restart, d, rank, next_rank); });
}

int32_t rwr_part_begin(rwr_graph *g, int32_t slab_lo, int32_t slab_hi, const int32_t *seeds, int32_t K, double d,
                       void *dev_x, int32_t *tile_seeds_out)
{
    g_err[0] = 0;
    if (!g || !seeds || !dev_x) { set_error("rwr_part_begin: NULL argument"); return RWR_E_INVALID; }
    return bound("rwr_part_begin", g, [&] { return part_begin(g, slab_lo, slab_hi, seeds, K, d, (double *)dev_x, tile_seeds_out); });
}

int32_t rwr_part_local_step(rwr_graph *g, const void *dev_x, void *dev_y, void *dev_r)
{
    g_err[0] = 0;
    if (!g || !dev_x || !dev_y || !dev_r) { set_error("rwr_part_local_step: NULL argument"); return RWR_E_INVALID; }
    return bound("rwr_part_local_step", g, [&] { return part_local_step(g, (const double *)dev_x, (double *)dev_y, (double *)dev_r); });
}

int32_t rwr_part_step(rwr_graph *g, const void *dev_x, void *dev_y, void *stream)
{
    g_err[0] = 0;
    if (!g || !dev_x || !dev_y || dev_x == dev_y) { set_error("rwr_part_step: NULL or aliasing argument"); return RWR_E_INVALID; }
    return bound("rwr_part_step", g, [&] { return part_step(g, (const double *)dev_x, (double *)dev_y, (hipStream_t)stream); });
}

int32_t rwr_part_finish_step(rwr_graph *g, void *dev_y, const void *dev_r)
{
    g_err[0] = 0;
    if (!g || !dev_y || !dev_r) { set_error("rwr_part_finish_step: NULL argument"); return RWR_E_INVALID; }
    return bound("rwr_part_finish_step", g, [&] { return part_finish_step(g, (double *)dev_y, (const double *)dev_r); });
}

int32_t rwr_part_rank(rwr_graph *g, void *dev_x, int32_t top_n, int64_t *ids, double *scores, int32_t *counts)
{
    g_err[0] = 0;
    if (!g || !dev_x || !ids || !scores || !counts) { set_error("rwr_part_rank: NULL argument"); return RWR_E_INVALID; }
    return bound("rwr_part_rank", g, [&] { return part_rank(g, (double *)dev_x, top_n, ids, scores, counts); });
}

int32_t rwr_get_stats(rwr_graph *g, rwr_stats *out)
{
    if (!g || !out) { set_error("rwr_get_stats: NULL argument"); return RWR_E_INVALID; }
    size_t sz = out->struct_size > 0 ? (size_t)out->struct_size : sizeof(rwr_stats);
    if (sz > sizeof(rwr_stats)) sz = sizeof(rwr_stats);
    rwr_stats s = g->stats;
    if (!sweep_ready(g)) s.sweep_k = s.sweep_blocks = s.sweep_wgs = s.sweep_partial = 0;   // (a rebuild drops the tables: undecided again)
    s.struct_size = (int32_t)sz;
    memcpy(out, &s, sz);
    return RWR_OK;
}

int32_t rwr_reset_stats(rwr_graph *g)
{
    if (!g) { set_error("rwr_reset_stats: NULL argument"); return RWR_E_INVALID; }
    rwr_stats &s = g->stats;
    s.spmm_ms = s.chain_ms = s.rank_ms = s.iterate_wall_ms = s.total_wall_ms = 0;
    s.spmm_launches = s.spmm_seed_steps = s.chain_launches = s.seeds_done = s.chain_redo_blocks = 0;
    s.spmm_dense_ms = 0;
    s.spmm_dense_launches = s.spmm_dense_seed_steps = 0;
    s.frontier_list_launches = 0;
    s.rank_fused_groups = s.rank_fused_fallbacks = 0;
    s.rank_pruned_rows = 0;
    s.rank_bound_ms = 0;
    s.x_clear_skipped = 0;
    s.entry_live_launches = 0;
    s.spmv_sweep_launches = s.spmv_hub_launches = s.spmv_binned_launches = 0;   // (sweep_*: the graph's geometry, kept)
    return RWR_OK;
}

}  // extern "C"
