// What the API drivers (recommend.hip, model.hip, partition.hip, restart.hip) need from iterate.hip (internal): the launchers of
// the step's kernels, the profile events of a call, one tile group's power iteration; the run-loop pieces the Model drivers share.
#pragma once
#include "column_ends.h"
#include "engine.h"
#include "rank.h"
#include "seed_row.h"
#include "step_plan.h"

#include <new>
#include <optional>

namespace rwr {

// One SpMM  Y = (1-d) P^T X  over tg tiles of G seeds.  Zin != nullptr: value-free form -- the kernels gather Zin (z of the
// current ranks) instead of X and read no weights; Zout (may be nullptr) receives the next z.  nz_in / nz_out: the frontier
// bitmaps of X / Y (first iterations), act: the rows the step can reach (k_mark_active).  hub_scan: see launch_spmv_exact.
// rows: every row, a tail level (a batch's last steps; X / Y / Z keep their n rows) or the tiles' frontier
// lists.  G = 1, skip_seed_row = false, seeds -> a device int32 holding -1: the link-only single-row SpMV.
// A row of a tile's candidate buffer and what the selecting launch appends to: slot = tile * G + lane; a lane whose
// row sum is >= tau[slot] takes position atomicAdd(cursor[slot], 1) of its slot's `stride` entries and stores (row, score)
// there while the position is below cap, else sets *overflow.  Integer atomics only.
struct RowScore {
    int32_t row, pad;
    double score;
};
struct SelSink {
    const double *tau = nullptr;
    int32_t *cursor = nullptr;
    RowScore *cand = nullptr;
    int32_t cap = 0, stride = 0;
    int32_t *overflow = nullptr;
    // pruned body (rank_bound_prepare): tile t walks the list_cnt[t] rows at list + t * list_stride instead of the launch's rows
    const int32_t *list = nullptr, *list_cnt = nullptr;
    int64_t list_stride = 0;
};

struct SpmmArgs {
    const double *X = nullptr;
    double *Y = nullptr;
    const int32_t *seeds = nullptr;
    double c1 = 0.0;
    bool skip_seed_row = false;   // the seed-row kernel writes the seeds' own rows
    const uint32_t *nz_in = nullptr;
    uint32_t *nz_out = nullptr;
    const uint32_t *act = nullptr;
    const double *Zin = nullptr;
    double *Zout = nullptr;
    bool hub_scan = false;
    RowSource rows{};
    int32_t row_first = 0, row_count = -1;   // a tail level's rows [row_first, row_first + row_count) only (-1: to the end)
    const SelSink *sel = nullptr;            // the launch writes no Y: it appends the rows that reach tau (k_spmm_select)
    // a probing launch over every row (nz_in set): the step's per-link tile masks [slab][nnz] (launch_entry_live), which it
    // reads instead of probing nz_in; nullptr: the bitmap probe
    const uint32_t *ent_live = nullptr;
};
void launch_spmm(rwr_graph *g, int G, int tg, const SpmmArgs &a, hipStream_t s);
// k_init_seeds (Model ctor), k_make_z (z of `elems` elements of X, w_src[0] belonging to X's first row), k_make_z_nz (z and
// non-zero bitmap of the slab rows [lo, hi)), k_mark_active (fl_rows / fl_cnt: the tiles' row lists, or nullptr)
void launch_init_seeds(rwr_graph *g, int G, int tg, double *X, const int32_t *seeds, uint32_t *nz, double *Z, double c1,
                       hipStream_t s);
void launch_make_z(int64_t elems, int G, const double *X, double *Z, const double *w_src, double c1, hipStream_t s);
void launch_make_z_nz(rwr_graph *g, int32_t lo, int32_t hi, int G, const double *X, double *Zs, double c1, uint32_t *nz,
                      hipStream_t s);
void launch_mark_active(rwr_graph *g, int G, int tg, const uint32_t *nz, uint32_t *act, const int32_t *seeds, int32_t *fl_rows,
                        int32_t *fl_cnt, hipStream_t s);

// Profile events of a call (opts.profile): begin / end pairs of the profiled stages, from a pool of events that fold()
// folds into rwr_stats and recycles after a synchronisation.  With profiling off every method does nothing.
struct Profile {
    const bool on;
    std::vector<hipEvent_t> pool, spmm, chain, rank, iter, bound;   // the pool; pairs of the SpMM, chain, ranking, iteration, body-bound stages
    size_t used = 0;                                          // (pool[0 .. used) are in flight)
    std::vector<uint8_t> dense;                               // per SpMM pair: 1 = a dense launch
    explicit Profile(const rwr_graph *g) : on(g->opts.profile != 0) {}
    ~Profile() { for (auto e : pool) (void)hipEventDestroy(e); }
    int32_t record(hipEvent_t &e, hipStream_t s);             // an event of the pool recorded on s: the begin of a pair
    int32_t end(std::vector<hipEvent_t> &stage, hipEvent_t a, hipStream_t s);   // the end of the pair that `a` began
    void reset() { spmm.clear(); chain.clear(); rank.clear(); iter.clear(); bound.clear(); dense.clear(); used = 0; }
    int32_t fold(rwr_graph *g);
};

// One tile group's power iteration: init() = Model ctor (Model.cs:33-50), step() = deliverRanks + updateRanks
// (Model.cs:76-108) as plan_step() (step_plan.h) decided it.  After step() `X` holds the new ranks and `Y` still holds the
// previous ones.
struct GroupIter {
    rwr_graph *g;
    int G, tg;
    const int32_t *d_seeds;
    const int64_t *d_evoff;
    double c1;
    double *X, *Y;
    double *Zc = nullptr, *Zn = nullptr;   // value-free path: z of the current ranks / of the ranks being produced
    uint32_t *nz_cur = nullptr, *nz_oth = nullptr;
    PlanConfig cfg;
    int64_t it = 0;
    int64_t dense_steps = 0;   // steps whose SpMM walked every row (no frontier bitmap)

    GroupIter(rwr_graph *g_, int G_, int tg_, const int32_t *seeds, const int64_t *evoff, double d)
        : g(g_), G(G_), tg(tg_), d_seeds(seeds), d_evoff(evoff), c1(1 - d) /* Model.cs:84: (1 - dampingFactor) */,
          X(g_->X.p), Y(g_->Y.p), Zc(g_->vf ? g_->Z0.p : nullptr), Zn(g_->vf ? g_->Z1.p : nullptr) {}

    // fresh = Model ctor (rank = n at the seed, 0 elsewhere);  !fresh = X already holds a caller-supplied rank vector
    // (Model.deliverRanks called on its own);  ranking_only: the caller (iterate_group) reads only the ranking
    int32_t init(bool fresh = true, bool ranks_nonneg = true, bool ranking_only = false);
    // row_first / row_count: a tail step over that part of its row list only
    int32_t step(const StepPlan &p, Profile &prof, int32_t row_first = 0, int32_t row_count = -1);
    // The step that has just run (a chainless tail step that forms no z), again over rows [row_first, row_first + row_count)
    // of its list: its inputs are the other ping-pong buffers, still intact.  sel: select instead of writing (SelSink)
    int32_t redo_rows(const StepPlan &p, Profile &prof, int32_t row_first, int32_t row_count, const SelSink *sel);
};

// A tile group of recommend_batch: T steps of the plan.  h_seeds: the group's tg * G seed slots on the host (-1 = padding),
// whose tail flags decide which of the last steps run their seed-row chain.
// split: head > 0 asks for the last step over the first `head` rows of tail_rows[0] only.  Granted (taken)
// when that step is a chainless, probe-free walk of tail level 0 by the chunked kernels; gi / last then let the caller run
// the rest of the step (GroupIter::redo_rows).
struct SplitLast {
    int32_t head = 0;
    bool taken = false;
    StepPlan last;
    std::optional<GroupIter> gi;   // out: the group's iterator after the head part
};
int32_t iterate_group(rwr_graph *g, int G, int tg, const int32_t *d_seeds, const int64_t *d_evoff, const int32_t *h_seeds,
                      double d, int64_t T, Profile &prof, double **final_X, int64_t *dense_steps, SplitLast *split = nullptr);

// recommend.hip: seeds per tile, the batch workspace (extra_mats: further [tile][n][G] matrices the caller needs per tile),
// the seeds dealt to tile slots (d_seeds, d_slot_k, d_evoff)
int resolve_G(const rwr_graph *g, int32_t K);
int32_t ensure_workspace(rwr_graph *g, int G, int32_t K, int *TG_out, int extra_mats = 0);
int32_t upload_seed_slots(rwr_graph *g, const int32_t *seeds, int32_t K, int G, std::vector<int32_t> *slot_k_out,
                          std::vector<int32_t> *slot_seed_out = nullptr);

// ---- the run loop of the Model drivers (model.hip, restart.hip, restart_batch.hip) ----------------------------------------
// Model.run of one walk (Model.cs:52-66): step() = deliverRanks + updateRanks, converge(&dist) = checkConvergence read
// back.  *done receives the steps made; a threshold run that is not below its threshold after end.T steps fails.
template <class Step, class Converge>
int32_t run_walk(const char *who, const RunEnd &end, int64_t *done, Step &&step, Converge &&converge)
{
    for (*done = 0; *done < end.T;) {
        RWR_TRY(step());
        ++*done;
        if (end.by_count) continue;
        double dist = 0;
        RWR_TRY(converge(&dist));
        if (dist < end.threshold) return RWR_OK;                     // Model.cs:64
    }
    if (end.by_count) return RWR_OK;
    set_error("%s: no convergence within %lld iterations (RWR_MAX_ITERS)", who, (long long)end.max_iters);
    return RWR_E_UNSUPPORTED;
}

// The device half of ColumnEnds (column_ends.h) for one tile group of K Models, on g->stream (model.hip).  The caller has
// sized g->mb_row and g->cs_sums to the group's slots and g->cs_diff to one [tile][n][G] matrix.
struct GroupColumns {
    rwr_graph *g;
    int G, tg;
    const int64_t *evoff;        // the group's d_evoff slots (chain_scan_sum_cols)
    double *rank_out;            // the call's K x n result: column k leaves as row k
    int64_t *iters_out;
    Profile &prof;
    ColumnEnds ends;
    std::vector<int32_t> row_of;
    std::vector<double> dist;    // threshold modes: the slots' distances of the last step
    GroupColumns(rwr_graph *g_, int G_, int tg_, const int32_t *slot_k, const int64_t *evoff_, const RunEnd &end, double *rank_out_,
                 int64_t *iters_out_, Profile &prof_)
        : g(g_), G(G_), tg(tg_), evoff(evoff_), rank_out(rank_out_), iters_out(iters_out_), prof(prof_),
          ends(slot_k, (size_t)tg_ * G_, end.by_count, end.T, end.threshold), row_of(ends.nslots), dist(ends.nslots) {}
    // The columns of X whose run ends after `steps` steps (ends.due(steps)) go to their caller rows: k_extract_cols into
    // cs_diff (booked as ranking time), one D2H per row, one synchronisation.  Nothing when no column leaves.
    int32_t emit(int64_t steps, const double *X);
    // checkConvergence of every column after a step (Model.cs:110-115): |Y - X| and its exact column sums close the iter
    // bracket that i0 began, then dist comes back with one synchronisation
    int32_t measure(hipEvent_t i0, const double *Y, const double *X);
    // the group is through after `steps` steps, dense_steps of them SpMMs over every row: its real columns' statistics
    void count(int64_t steps, int64_t dense_steps) const
    {
        g->stats.spmm_seed_steps += (int64_t)ends.real * steps;
        g->stats.spmm_dense_seed_steps += (int64_t)ends.real * dense_steps;
    }
};
// The end of a batch call: both streams idle, the profile folded, the tile shape and the wall time since t_begin booked
int32_t finish_model_batch(rwr_graph *g, Profile &prof, int G, int TG, double t_begin);

}  // namespace rwr
