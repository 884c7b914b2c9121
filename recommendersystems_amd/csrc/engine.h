// Device-resident graph and batch workspace (internal).
#pragma once
#include <chrono>
#include <cstdlib>
#include <new>

#include "cand_plan.h"
#include "common.h"
#include "stage_layout.h"
#include "typed_call.h"

struct rwr_graph {
    int32_t device = 0;
    int32_t n = 0;
    int64_t nnz_raw = 0;     // links handed over
    int64_t nnz = 0;         // explicit links = entries of the transition matrix
    int32_t n_items = 0;     // nodes of type ITEM
    uint64_t id_key_top = 0; // largest ITEM id (order-preserving unsigned form) and the bits of the id range: sort keys of item_order
    int32_t id_key_bits = 64;
    uint64_t id_key_lo = 0;  // smallest ITEM id in the same form, once rwr_graph_append_nodes has read it back (id_key_lo_known): the
    int32_t id_key_lo_known = 0;   // build keeps only the range's bit count, and a grown id set needs the range itself
    int32_t uniform = 0;     // every row's explicit raw weights equal
    // Value-free matrix path (uniform && nonneg, RWR_VALUE_FREE != 0).  Every out-link of source i then carries the SAME
    // normalised weight w_src[i] (Graph.cs:79-81 divides equal raw weights by one sum), so the product Model.cs:87 adds,
    //     fl( fl((1-d) * rank[i]) * weight ),
    // is one and the same double for all links of i: it is formed once per node and step (z[i], written by the kernel
    // that produced rank[i]) and the SpMM / SpMV gather z and read NO per-entry value -- 4 instead of 12 matrix bytes per
    // entry and one add per entry, bit for bit the reference's sums.  in_w is not even built on such graphs
    // (ensure_in_w materialises it for the few entry points that still take the weighted kernels).
    int32_t vf = 0;
    int32_t nonneg = 1;      // every normalised weight is a finite number >= 0 (raw weights >= 0, row sums in (0, inf)): ranks stay
                             // >= 0, which the zero-skipping frontier paths and the binade scan rely on; otherwise the general kernels run
    int32_t max_in_deg = 0;
    int32_t staged = 0;      // ego-network-sized graph: raw arrays arrived through the pinned staging buffer (stage_layout.h)
    int32_t stage_pending = 0;   // ... and the device-side copy of that buffer has not been unpacked into the arrays yet
    int32_t poisoned = 0;    // a failed incremental rebuild left raw and derived arrays out of step: every entry point refuses
    // rows of row_order (in-degree descending) with in-degree >= 128 / >= 32 / >= 4: lane-width bins of the K = 1 vector SpMV
    int32_t bin_end[3] = {0, 0, 0};
    int32_t bin_huge = 0;    // rows with in-degree >= 2048
    rwr_opts opts{};

    // node SoA (struct Node, Graph.cs:4-17)
    rwr::DevBuf<int64_t> node_id;
    rwr::DevBuf<uint8_t> node_type;
    // raw out-links in list order (struct ForwardLink, Graph.cs:19-35); kept for the
    // exclusion list, which reads the RAW list (Recommender.cs:20-24)
    rwr::DevBuf<int64_t> rowptr;
    rwr::DevBuf<int32_t> dst;
    rwr::DevBuf<uint8_t> etype;
    rwr::DevBuf<double> w_raw;        // raw weights as handed over (kept for incremental rebuilds)
    rwr::DevBuf<double> w_norm_raw;   // Graph.graph weights per raw link (0 for UNDEFINED)
    std::vector<int64_t> h_rowptr;    // host copy (seed validation, exclusion sizing)
    std::vector<uint8_t> h_dangling;  // host copy of dangling[] (dangling seeds are answered without iterating)
    std::vector<int64_t> h_in_ptr;    // host copy of in_ptr (sizing of the seeds' in-link term buffers)
    // transposed (in-neighbour) CSR of the normalised matrix, entries ordered
    // (source asc, list position asc) = addend order of Model.deliverRanks
    rwr::DevBuf<int64_t> in_ptr;
    rwr::DevBuf<int32_t> in_src;
    rwr::DevBuf<double> in_w;
    rwr::DevBuf<double> w_src;        // uniform graphs: the one normalised weight of source i
    rwr::DevBuf<uint8_t> dangling;    // graph[i] == null (Graph.cs:53,86)
    rwr::DevBuf<int32_t> row_order;   // destination rows by in-degree descending (stable)
    // single-seed SpMV: ITEM rows first, then the rest, each by in-degree descending.  An item's in-links come from users and
    // a user's mostly from items, so each phase gathers from one region of the rank vector and the XCDs' L2s are not split
    // between the two regions; x_rows[p] = rows of phase p, x_bins[p][0..2] = how many of them have >= 128 / 32 / 4 in-links
    rwr::DevBuf<int32_t> row_order_x;
    int32_t x_rows[2] = {0, 0};
    int32_t x_bins[2][3] = {{0, 0, 0}, {0, 0, 0}};
    int32_t x_hub[2] = {0, 0};        // rows of phase p with in-degree >= hub_t (hub rows of the exact single-seed SpMV)
    int32_t bin_hub = 0, hub_t = 2048; // ... and of the one-phase order; the threshold (RWR_HUB_T)
    std::vector<uint8_t> h_is_item;
    rwr::DevBuf<int32_t> item_order;  // ITEM rows by id descending
    rwr::DevBuf<int32_t> item_rows;   // ITEM rows by row index ascending
    // rows the ranking depends on in a batch's last steps, each in row_order's order: tail_rows[0] = the ITEM
    // rows, tail_rows[k] = every row with an explicit link into a row of tail_rows[k - 1], for k < tail_depth <= TAIL_MAX
    // (at most n x 4 B per level).  h_tail_flag[i] bit k: a seed at row i needs its seed-row chain at step T - k (bit 0: i is
    // an ITEM row; bit 1: i has an explicit raw link into an ITEM row it does not LIKE; bit k >= 2: i is in tail_rows[k]).
    // Built on first use (tail_rows_prepare), dropped by every (re)build: tail_state 0 = not built, 1 = built
    static constexpr int TAIL_MAX = 4;
    rwr::DevBuf<int32_t> tail_rows[TAIL_MAX];
    int32_t tail_n[TAIL_MAX] = {0, 0, 0, 0};
    int32_t tail_depth = 0;
    std::vector<uint8_t> h_tail_flag;
    int32_t tail_state = 0;
    // candidate rows by node type (rwr_recommend_typed_batch): cand_rows[e] = the rows with node_type ==
    // cand_entry[e].type by row index ascending, compacted on the device on first use (typed.hip).  An entry is valid while
    // cand_entry[e].n == n (cand_plan.h: node types never change, and between two removals nodes are only appended), so no
    // (re)build resets it; rwr_graph_remove_nodes, after which the same n can stand for other rows, empties every entry
    rwr::DevBuf<int32_t> cand_rows[rwr::CAND_CACHE];
    rwr::CandEntry cand_entry[rwr::CAND_CACHE];
    uint64_t cand_calls = 0;          // typed calls so far: the entries' use stamps

    // single-seed SpMV of value-free graphs as a source-block sweep with z staged through LDS (sweep.hip): 0 = not decided
    // yet, 1 = tables built, -1 = this graph does not qualify; re-decided after every (re)build
    int32_t sw_state = 0, sw_B = 0, sw_BN = 0, sw_K = 0, sw_nwg = 0, sw_wpg = 0, sw_hub0 = 0;
    int32_t sw_rows = 0;              // rows the sweep serves (all non-hub rows, or -- sw_partial -- the non-hub ITEM rows only)
    int32_t sw_partial = 0;           // 1: phase 0 (ITEM rows) by the sweep, phase 1 by the row-binned kernel beside it
    rwr::DevBuf<uint32_t> sw_wgblk;   // [workgroup][block]: does any row of the workgroup read that block (else its refill is skipped)
    int64_t sw_words = 0;             // 64-bit words of the entry stream (4 block-local 16-bit indices each)
    rwr::DevBuf<int32_t> sw_order;    // rows in sweep order (row_order_x without its hub rows)
    rwr::DevBuf<uint4> sw_meta;       // [wave][block]: first word-row of the chunk, piece lengths of the wave's slots
    rwr::DevBuf<uint2> sw_ent;        // the matrix in sweep order

    // batch workspace (lazily sized)
    rwr::DevBuf<double> X, Y;         // rank matrices [tile][n][G]
    rwr::DevBuf<int32_t> sm_tab;      // small.hip: places of the seed row's addends (per call)
    void *sm_pin = nullptr;           // small.hip: pinned host buffer the one-launch kernel writes the ranked list into
    void *sm_stage = nullptr;         // stage_layout.h: pinned staging buffer of an ego-network-sized graph's upload / read-back
    // a handle built as part of a batch (rwr_eval_graphs, eval_graphs.hip; graphs_build_multi in build_small.hip, recommend_small_multi in
    // small.hip): its staging slot and read-back area lie in the batch's pinned arena, the device-side landing area in the
    // batch's one buffer (one H2D copy for all graphs); none of them is owned by the handle
    uint8_t *sm_out = nullptr;
    const uint8_t *stage_dev_ext = nullptr;
    rwr::DevBuf<uint8_t> d_stage;     // ... and its device-side landing area
    int32_t sm_pin_count = -1;        // >= 0: the last single-seed call left its list (that many entries) in sm_pin
    rwr::DevBuf<double> Z0, Z1;       // value-free path: z = ((1-d) x) * w_src of the current / next ranks, same layout
    rwr::DevBuf<int32_t> d_seeds;     // [tile][G], -1 = padding lane
    rwr::DevBuf<int32_t> d_slot_k;    // [tile][G]: batch position of the seed in this slot (-1 = padding)
    rwr::DevBuf<double> d_part;       // partial sums of the deterministic tree reductions (global model, row-partitioned restart mass)
    rwr::DevBuf<unsigned int> d_gate;   // exact mode: check-in counter of the resident chain workgroups
    rwr::DevBuf<uint32_t> d_nz;       // [2][tile][ceil(n/32)] bitmaps: row of X / Y has a non-zero (first iterations)
    rwr::DevBuf<int32_t> fl_rows;     // [tile][n] frontier row lists of a batch's first steps, then [tile] their lengths
    // per-link tile masks of a batch's bitmap-probing steps, rewritten by every such step: ent_nzT =
    // [slab][n] the group's frontier bitmaps node-major (bit t & 31 of slab t >> 5 = node live in tile t), ent_live =
    // [slab][nnz] that word of every link's source, in the order of in_src
    rwr::DevBuf<uint32_t> ent_nzT, ent_live;
    rwr::DevBuf<int64_t> d_evoff;     // exact mode: per seed slot, offset of its in-link terms in d_evterm
    rwr::DevBuf<double> d_evterm;     // exact mode: ((1-d) x_src) * w of every link INTO a seed, list order
    // exact mode, parallel seed-row chain (chain_scan.hip): per (tile, block, seed) approximate block sum,
    // predicted biased exponent, parity-function pair; per (slot, block) offset into the seed's in-link list
    rwr::DevBuf<double> cs_approx;
    rwr::DevBuf<int32_t> cs_e;
    rwr::DevBuf<long long> cs_d0, cs_d1;
    rwr::DevBuf<double> cs_side;      // single seed: CS_SIDE_WORDS words per block (chain_scan.hip)
    rwr::DevBuf<double> cs_mx;        // single seed: scratch row of the exact-start block's addend sequence
    rwr::DevBuf<int32_t> cs_lnk;
    rwr::DevBuf<int32_t> cs_lnk0;     // all-zero link table + slot for chain_scan_sum (checkConvergence)
    rwr::DevBuf<double> cs_diff;      // |rank - nextRank| per node (checkConvergence); rwr_model_run_batch: [tile][n][G], the
                                      // tile group's differences and, between steps, the row-major staging of extracted columns
    rwr::DevBuf<double> cs_sums;      // rwr_model_run_batch: per (tile, slot) sum of the differences, the G-wide checkConvergence
    rwr::DevBuf<int32_t> mb_row;      // rwr_model_run_batch: per (tile, slot) staging row of a column extracted now, -1 = none
    rwr::DevBuf<unsigned long long> cs_redo;   // blocks redone by the carry kernel (binade crossings + mispredictions)
    rwr::DevBuf<uint64_t> keys, keys_alt;
    rwr::DevBuf<uint32_t> vals, vals_alt;
    rwr::DevBuf<uint8_t> sort_temp;
    rwr::DevBuf<uint8_t> fused_ws;    // ranking inside the last step: per slot tau, append cursor, candidates
    rwr::DevBuf<uint8_t> bound_ws;    // ... pruning its body: the tiles' bound tables, the rows' keep bits, flags and counters
    int32_t bound_first = -1, bound_lo = 0, bound_hi = 0;   // source rows [lo, hi) of the in-links of tail_rows[0] from bound_first
                                                            // on (-1: not known; reset whenever the tail rows are rebuilt)
    rwr::DevBuf<int64_t> d_out_id;
    rwr::DevBuf<double> d_out_score;
    rwr::DevBuf<int32_t> d_counts;

    // row-partitioned mode (rwr_part_*)
    int32_t part_lo = 0, part_hi = 0, part_G = 0, part_K = 0;
    int32_t part_steps = 0;           // slab steps since rwr_part_begin (the first ones mark the frontier, like the seed path)
    double part_c1 = 0;
    std::vector<int32_t> part_seeds;

    hipStream_t stream = nullptr, stream2 = nullptr;
    hipStream_t stream3 = nullptr;    // hub rows of the exact single-seed SpMV, beside the binned kernel
    hipEvent_t ev_h0 = nullptr, ev_h1 = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    hipEvent_t ev_a = nullptr, ev_b = nullptr, ev_c = nullptr, ev_d = nullptr;   // profiling pairs

    rwr_stats stats{};
};

namespace rwr {

// CALL with GG = the tile width G as a constant expression (a power of two <= 64)
#define RWR_DISPATCH_G(G, CALL)                          \
    switch (G) {                                         \
        case 1: { constexpr int GG = 1; CALL; } break;   \
        case 2: { constexpr int GG = 2; CALL; } break;   \
        case 4: { constexpr int GG = 4; CALL; } break;   \
        case 8: { constexpr int GG = 8; CALL; } break;   \
        case 16: { constexpr int GG = 16; CALL; } break; \
        case 32: { constexpr int GG = 32; CALL; } break; \
        default: { constexpr int GG = 64; CALL; } break; \
    }

double now_ms();   // recommend.hip: a steady clock, for the wall times of rwr_stats

// The experiments build's wall-clock stamps of a host function's stages, for tools/*_latency.py: one object per switch at
// file scope -- Stamps("append", "RWR_APPEND_TIMING"), which reads the variable once, through RWR_TUNE_ENV -- and one copy per
// call, begin(), which keeps the time of the call's last stamp.  stamp("label") prints the microseconds since then to stderr
// as "[tag] label  us".  In the shipped library on() is a constant false and every stamp compiles to nothing.
class Stamps {
public:
    Stamps(const char *tag, const char *env_name) : tag_(tag)
    {
        const char *e = RWR_TUNE_ENV(env_name);
        on_ = e && atoi(e) != 0;
    }
#ifdef RWR_EXPERIMENTS
    bool on() const { return on_; }
#else
    bool on() const { return false; }
#endif
    static double now()                // microseconds of a steady clock
    {
        using namespace std::chrono;
        return duration<double, std::micro>(steady_clock::now().time_since_epoch()).count();
    }
    Stamps begin() const
    {
        Stamps s = *this;
        s.t_ = on() ? now() : 0.0;
        return s;
    }
    void operator()(const char *label)
    {
        if (!on()) return;
        const double t = now();
        fprintf(stderr, "[%s] %-28s %8.1f us\n", tag_, label, t - t_);
        t_ = t;
    }

private:
    const char *tag_;
    bool on_ = false;
    double t_ = 0.0;
};

// scratch buffers of one call are released only after both streams are idle (also on error paths): declared after them
struct StreamsIdle {
    rwr_graph *g;
    ~StreamsIdle() { (void)hipStreamSynchronize(g->stream); (void)hipStreamSynchronize(g->stream2); }
};

// ... and of a function that launches on one stream and ends in its own synchronisation: `body`, run with the scratch buffers
// declared before it, may leave through RWR_HIP / RWR_TRY between a launch and that synchronisation; the stream is then drained
// here, before the caller's scratch goes back to the block cache.  A body that returns RWR_OK costs nothing more.
template <class F>
int32_t idle_on_error(hipStream_t s, F &&body)
{
    const int32_t rc = body();
    if (rc != RWR_OK) (void)hipStreamSynchronize(s);
    return rc;
}

// two buffers change places: how an edit of the resident graph hands a NEW buffer to the handle (edit.h: StagedLinks and
// StagedNodes group the exchanges of the three edit drivers); the old one goes back to the block cache when the edit's locals
// go out of scope
template <typename T>
void swap_blocks(DevBuf<T> &a, DevBuf<T> &b)
{
    T *tp = a.p; a.p = b.p; b.p = tp;
    size_t tc = a.count; a.count = b.count; b.count = tc;
    size_t tr = a.reserved; a.reserved = b.reserved; b.reserved = tr;
}

// no C++ exception crosses the C boundary
template <class F>
int32_t no_throw(const char *who, F &&body)
{
    try { return body(); }
    catch (const std::bad_alloc &) { set_error("%s: host allocation failed", who); return RWR_E_NOMEM; }
    catch (...) { set_error("%s: unexpected host exception", who); return RWR_E_HIP; }
}

// Node count from which a graph counts as "beyond the L2s" (its rank vector no longer fits them): two-phase row order of
// the single-seed SpMV, one more frontier iteration, 32-seed tiles.
// RWR_BIG_N overrides the default of 2 M so that small test graphs can reach the same code paths.
inline int32_t spmv_big_n()
{
    static const int32_t v = [] { const char *e = getenv("RWR_BIG_N"); return e ? (int32_t)atol(e) : (int32_t)2000000; }();
    return v;
}

int32_t graph_build(rwr_graph *g, const int64_t *node_id, const uint8_t *node_type, const int64_t *rowptr,
                    const int32_t *dst, const uint8_t *etype, const double *w);

int32_t graph_update_links(rwr_graph *g, int64_t count, const int64_t *idx, const uint8_t *etype, const double *w);
// rwr_graph_append_links (n_new == 0) and rwr_graph_append_nodes: grows the node arrays by n_new nodes with empty lists, merges
// the links into the resident raw lists (new buffers, swapped in when all of them exist: *swapped) and re-derives; the plans are
// node_append_plan.h's and append_plan.h's.  `who` names the entry point in the messages.
int32_t graph_append(rwr_graph *g, const char *who, int32_t n_new, const int64_t *node_id, const uint8_t *node_type,
                     int64_t count, const int32_t *src, const int32_t *dst, const uint8_t *etype, const double *w,
                     int64_t *new_index_out, bool *swapped);
// rwr_graph_remove_links (remove.hip): compacts the resident raw lists without the links at the given positions
// (new buffers, swapped in when all of them exist: *swapped) and re-derives; the plan is remove_plan.h's.
int32_t graph_remove(rwr_graph *g, int64_t count, const int64_t *link_index, bool *swapped);
// rwr_graph_remove_nodes (node_remove.hip): compacts the resident raw lists without the links from or to the given
// nodes, renumbers the targets, compacts the node arrays and the ITEM orders (new buffers, swapped in when all of them exist:
// *swapped) and re-derives; the plan is node_remove_plan.h's.  The three outputs (each may be NULL) are written on success only.
int32_t graph_remove_nodes(rwr_graph *g, int32_t count, const int32_t *node_index, int32_t *new_node_index_out,
                           int64_t *new_link_index_out, int64_t *links_removed_out, bool *swapped);
// value-free graphs: materialise in_w (= w_src[in_src]) for an entry point that runs the weighted kernels
int32_t ensure_in_w(rwr_graph *g);
// sort.hip: m sorted payload words as the int32 row list their readers take (no launch for m <= 0)
void launch_u32_to_i32(const uint32_t *a, int32_t *b, int64_t m, hipStream_t s);
// tail_rows.hip: g->tail_rows / tail_n / tail_depth / h_tail_flag of the current matrix (built once per (re)build)
int32_t tail_rows_prepare(rwr_graph *g);
// build_small.hip: does a graph take the staged upload and the one-launch build (stage_layout.h: the limits)
bool graph_fits_small_build(int32_t n, int64_t m);
// many ego-network-sized graphs at once (rwr_eval_graphs): one build launch, one call launch, one evaluation launch
// (pool.hip: the thread's pinned buffers)
void multi_pins_acquire();    // a set of pinned buffers for this thread's rwr_eval_graphs call (from a process-wide pool) ...
void multi_pins_release();    // ... and back
int32_t multi_pinned(int slot, size_t bytes, void **out);   // buffer number `slot` (0..5) of the acquired set, at least `bytes` long
int32_t graphs_build_multi(rwr_graph **gs, int32_t count, const rwr_graph_desc *descs, const int32_t *caller_index, hipStream_t s);
int32_t recommend_small_multi(rwr_graph **gs, const int32_t *seeds, int32_t count, double d, int32_t n_iter, hipStream_t s,
                              rwr::DevBuf<uint8_t> &args_keep);
int32_t eval_ranked_multi(rwr_graph **gs, int32_t count, const int64_t *test_ptr_host, const int64_t *test_sorted_host,
                          int64_t *n_hits, double *sum_precision, int64_t *list_len, hipStream_t s);
// eval_graphs.hip: the driver of rwr_eval_graphs over the three above (arguments as checked, outputs as zeroed by the entry point)
int32_t eval_graphs(int32_t count, const rwr_graph_desc *graphs, const int32_t *seeds, float d, int32_t n_iter,
                    const int64_t *test_ptr, const int64_t *test_ids, const rwr_opts *opts, int64_t *n_hits,
                    double *sum_precision, int64_t *list_len);

// recommend.hip: runs the power iteration for K seeds and leaves, per seed, the ranked list
// (mode 0: top-k into host arrays; mode 1: full rank vector of one seed)
int32_t recommend_batch(rwr_graph *g, const int32_t *seeds, int32_t K, double d, int32_t n_iter, int32_t top_n,
                        int64_t *ids, double *scores, int32_t *counts, int64_t row_stride);
// ... the K_all x top_n lists of g->d_out_id / d_out_score / d_counts into the caller's arrays (host rows row_stride wide)
int32_t copy_lists_back(rwr_graph *g, int32_t K_all, int32_t top_n, int64_t *ids, double *scores, int32_t *counts,
                        int64_t row_stride);
int32_t eval_ranked(rwr_graph *g, int32_t cnt, const int64_t *test_sorted_host, int64_t n_test, int64_t *n_hits,
                    double *sum_precision);
int32_t eval_ranked_batch(rwr_graph *g, int32_t K, int64_t row_stride, const int64_t *test_ptr_host,
                          const int64_t *test_sorted_host, int64_t *n_hits, double *sum_precision);
// partition.hip: the row-partitioned mode (rwr_part_*)
int32_t part_begin(rwr_graph *g, int32_t lo, int32_t hi, const int32_t *seeds, int32_t K, double d, double *x,
                   int32_t *G_out);
int32_t part_local_step(rwr_graph *g, const double *x, double *y, double *r);
int32_t part_step(rwr_graph *g, const double *x, double *y, hipStream_t stream);
int32_t part_finish_step(rwr_graph *g, double *y, const double *r);
int32_t part_rank(rwr_graph *g, double *x, int32_t top_n, int64_t *ids, double *scores, int32_t *counts);
// model.hip: Model.run / deliverRanks (seed -1: the global model)
int32_t model_run(rwr_graph *g, int32_t seed, double d, int32_t run_mode, double value, double *rank_out,
                  int64_t *iters_out);
int32_t model_deliver(rwr_graph *g, int32_t seed, double d, const double *rank_in, double *next_out);
// K personalised Models in one call (rwr_model_run_batch): row k of rank_out / iters_out[k] as model_run for seeds[k]
int32_t model_run_batch(rwr_graph *g, const int32_t *seeds, int32_t K, double d, int32_t run_mode, double value,
                        double *rank_out, int64_t *iters_out);
// restart.hip: Model with a caller-set restart vector (rwr_model_run_restart / rwr_model_deliver_restart)
int32_t model_run_restart(rwr_graph *g, const double *v, const double *rank_in, double d, int32_t run_mode, double value,
                          double *rank_out, int64_t *iters_out);
int32_t model_deliver_restart(rwr_graph *g, const double *v, double d, const double *rank_in, double *next_out);
// restart_batch.hip: K Models with caller-set restart vectors in one call (rwr_model_run_restart_batch).  The
// vectors arrive as validated CSR (api.hip, check_restart_vectors: indices in range and distinct, values finite, start in [-1, n) or NULL)
int32_t model_run_restart_batch(rwr_graph *g, int32_t K, const int64_t *sup_ptr, const int32_t *sup_idx, const double *sup_val,
                                const int32_t *start, double d, int32_t run_mode, double value, double *rank_out,
                                int64_t *iters_out);
// ... and the same walks ranked on the device (rwr_recommend_restart_batch): the top_n candidates of every vector,
// the raw LIKE links of the members of set k (set_ptr / set_idx, validated by exclude_check) excluded; T steps, values >= 0
int32_t recommend_restart_batch(rwr_graph *g, int32_t K, const int64_t *sup_ptr, const int32_t *sup_idx, const double *sup_val,
                                const int32_t *start, const int64_t *set_ptr, const int32_t *set_idx, double d, int32_t n_iter,
                                int32_t top_n, int64_t *ids, double *scores, int32_t *counts);
// ... or evaluated there (rwr_recommend_restart_eval_batch): Hits / average precision of every vector's list, cut
// to top_n when top_n > 0, against test set k (test_ptr / test_ids, validated by eval_check) -- by counting, no list is written
int32_t recommend_restart_eval_batch(rwr_graph *g, int32_t K, const int64_t *sup_ptr, const int32_t *sup_idx, const double *sup_val,
                                     const int32_t *start, const int64_t *set_ptr, const int32_t *set_idx, double d, int32_t n_iter,
                                     int32_t top_n, const int64_t *test_ptr, const int64_t *test_ids, int64_t *n_hits,
                                     double *sum_precision, int64_t *list_len);
// ... and its kernels (restart.hip, beside the fold they share with the single call).  Pair j = support row pr[j] with
// restart value pv[j] of the vector in slot pq[j] = tile * G + lane of the group's X[tile][n][G]; fold[j] receives the
// row's next rank; st[slot]: the constructor's start node, -1 = every rank 1, -2 = padding slot
void launch_restart_fold_cols(rwr_graph *g, int G, int32_t npairs, const int32_t *pq, const int32_t *pr, const double *pv,
                              const double *X, double c1, double *fold, hipStream_t s);
void launch_restart_scatter_cols(rwr_graph *g, int G, int32_t npairs, const int32_t *pq, const int32_t *pr, const double *fold,
                                 double *Y, hipStream_t s);
void launch_restart_init_cols(rwr_graph *g, int G, int tg, const int32_t *st, double *X, hipStream_t s);
// typed.hip: the one driver of the eight seed-driven typed entries (rwr_recommend_typed_batch, _typed_eval_batch,
// _typed_positions_batch, _filtered_batch, _filtered_positions_batch, _capped_batch, _capped_positions_batch, _explained_batch;
// DESIGN §3.16-3.22).  K personalised walks of T whole steps ranked among the call's candidates -- the rows of cand_type (-1:
// of any type) that the pool lists -- the seed's raw out-links whose type has its bit in excl_edge_mask excluded, the seed too
// when exclude_self, the rows of deny list k dropped, at most group_cap candidates per group kept; then the destination the
// call names.  `call` as typed_call.h's typed_call_check passed it, a nonneg graph and d in [0, 1]; `who` names the entry
int32_t typed_body(rwr_graph *g, const TypedCall &call, double d, int32_t n_iter, const char *who);
// ... and the candidates restart_batch.hip's typed end shares with it: the device list of the rows with node_type == type,
// ascending, cached per handle (cand_plan.h); call it on an idle stream and before the workspace is sized.  (The end of a
// tile group itself -- exclusion, ranking or evaluation, copy-back -- is ranked_end.h's, for both drivers.)
int32_t cand_rows_get(rwr_graph *g, int32_t type, const int32_t **rows, int32_t *nrows);
// ... the restart-vector walks of rwr_recommend_restart_batch ranked among the nodes of one type
// (rwr_recommend_restart_typed_batch): top_n <= the select path's limit
int32_t recommend_restart_typed_batch(rwr_graph *g, int32_t K, const int64_t *sup_ptr, const int32_t *sup_idx,
                                      const double *sup_val, const int32_t *start, const int64_t *set_ptr, const int32_t *set_idx,
                                      double d, int32_t n_iter, int32_t top_n, int32_t cand_type, uint32_t excl_edge_mask,
                                      int32_t exclude_members, int64_t *ids, double *scores, int32_t *counts);
// ... and the positions and scores of test ids in their WHOLE lists (rwr_recommend_restart_typed_positions_batch, DESIGN
// §3.19): eval_count.hip's counting, finished by eval_pos.hip
int32_t recommend_restart_typed_positions_batch(rwr_graph *g, int32_t K, const int64_t *sup_ptr, const int32_t *sup_idx,
                                                const double *sup_val, const int32_t *start, const int64_t *set_ptr,
                                                const int32_t *set_idx, double d, int32_t n_iter, int32_t cand_type,
                                                uint32_t excl_edge_mask, int32_t exclude_members, const int64_t *test_ptr,
                                                const int64_t *test_ids, int64_t *pos_out, double *score_out, int64_t *list_len);
// model.hip pieces restart.hip runs as well (the loops around them: run_walk and GroupColumns, iterate.h).  A run's end condition (Model.run(int) / run(double) / run(), Model.cs:52-66):
// T steps at most; !by_count: until checkConvergence's distance is < threshold, a failure after max_iters = RWR_MAX_ITERS steps
struct RunEnd {
    bool by_count;
    double threshold;
    int64_t T, max_iters;
    RunEnd(int32_t run_mode, double value, int32_t n);
};
int64_t model_max_iters();
// the tree-summed restart mass and |a - b| sums into *total (partials in g->d_part[0, MODEL_RED_PARTS), which the caller
// sizes to MODEL_RED_PARTS + 8: model_scalar() is the cell behind the partials), |a - b| per node
constexpr int MODEL_RED_PARTS = 256;
inline double *model_scalar(rwr_graph *g) { return g->d_part.p + MODEL_RED_PARTS; }
void launch_restart_mass(rwr_graph *g, const double *X, double c1, double *total, hipStream_t s);
void launch_l1(rwr_graph *g, const double *a, const double *b, int32_t n, double *total, hipStream_t s);
void launch_absdiff(const double *a, const double *b, int32_t n, double *out, hipStream_t s);
// checkConvergence (Model.cs:110-115) of two rank vectors on g->stream, read back (one synchronisation): the reference's
// sequential sum bit for bit (binade scan), or the tree sum (tolerance parity: global model, wide restart vectors)
int32_t converge_exact(rwr_graph *g, const double *a, const double *b, double *dist);
int32_t converge_tree(rwr_graph *g, const double *a, const double *b, double *dist);
// spmv.hip: single-seed SpMV (list-order sums, rows binned by in-degree)
// (zin != nullptr: value-free form -- gathers zin, reads no per-entry value; zout (may be nullptr) receives the next z)
// (hub_scan: every addend is known to be >= 0 and finite -- weights, ranks and 1-d -- so that rows of >= 2048 in-links may
//  be summed by the exact parallel reduction of pf.h instead of one add at a time)
void launch_spmv_exact(rwr_graph *g, const double *X, double *Y, const int32_t *seeds, double c1, int skip,
                       const uint32_t *act, uint32_t *nz_out, hipStream_t s, const double *zin = nullptr,
                       double *zout = nullptr, bool hub_scan = false);
// sweep.hip: single-seed SpMV of value-free graphs, z staged through LDS source block by source block (bitwise the same sums)
int32_t sweep_prepare(rwr_graph *g);
bool sweep_ready(const rwr_graph *g);
void launch_sweep(rwr_graph *g, const double *zin, double *Y, double *zout, const int32_t *seeds, int skip, double c1,
                  hipStream_t s);
// small.hip: ego-network-sized graphs, one single-seed Recommendation as ONE kernel launch (bitwise the EXACT path's result)
int32_t small_pin_ensure(rwr_graph *g);
void *small_pin_scratch(rwr_graph *g);   // the score half of the pinned result buffer (SM_MAX_ITEMS 8-byte words), as scratch
int64_t small_pin_words();
bool small_path_ok(const rwr_graph *g);
bool small_path_seed_ok(const rwr_graph *g, int32_t seed);
const int64_t *small_pin_ids(const rwr_graph *g);      // the list of the last recommend_small call, in pinned host memory
const double *small_pin_scores(const rwr_graph *g);
int32_t recommend_small(rwr_graph *g, int32_t seed, double d, int32_t n_iter, int32_t top_n, int64_t *ids, double *scores,
                        int32_t *count);
// (the exact seed-row chain -- the folds and the binade scan -- is declared in seed_row.h)

}  // namespace rwr
