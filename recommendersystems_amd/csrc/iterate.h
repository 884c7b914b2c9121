// What the API drivers (recommend.hip, model.hip, partition.hip, restart.hip) need from iterate.hip (internal): the
// launchers of the step's kernels, the profile events of a call and one tile group's power iteration.
#pragma once
#include "engine.h"
#include "step_plan.h"

namespace rwr {

// One SpMM  Y = (1-d) P^T X  over tg tiles of G seeds.  Zin != nullptr: value-free form -- the kernels gather Zin (z of the
// current ranks) instead of X and read no weights; Zout (may be nullptr) receives the next z.  nz_in / nz_out: the frontier
// bitmaps of X / Y (first iterations), act: the rows the step can reach (k_mark_active).  hub_scan: see launch_spmv_exact.
// rows: every row, a tail level (a batch's last steps; X / Y / Z keep their n rows) or the tiles' frontier
// lists.  G = 1, skip_seed_row = false, seeds -> a device int32 holding -1: the link-only single-row SpMV.
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
    std::vector<hipEvent_t> pool, spmm, chain, rank, iter;   // the pool; pairs of the SpMM, chain, ranking, iteration stages
    size_t used = 0;                                          // (pool[0 .. used) are in flight)
    std::vector<uint8_t> dense;                               // per SpMM pair: 1 = a dense launch
    explicit Profile(const rwr_graph *g) : on(g->opts.profile != 0) {}
    ~Profile() { for (auto e : pool) (void)hipEventDestroy(e); }
    int32_t record(hipEvent_t &e, hipStream_t s);             // an event of the pool recorded on s: the begin of a pair
    int32_t end(std::vector<hipEvent_t> &stage, hipEvent_t a, hipStream_t s);   // the end of the pair that `a` began
    void reset() { spmm.clear(); chain.clear(); rank.clear(); iter.clear(); dense.clear(); used = 0; }
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
    int32_t step(const StepPlan &p, Profile &prof);
};

// A tile group of recommend_batch: T steps of the plan.  h_seeds: the group's tg * G seed slots on the host (-1 = padding),
// whose tail flags decide which of the last steps run their seed-row chain.
int32_t iterate_group(rwr_graph *g, int G, int tg, const int32_t *d_seeds, const int64_t *d_evoff, const int32_t *h_seeds,
                      double d, int64_t T, Profile &prof, double **final_X, int64_t *dense_steps);

// recommend.hip: seeds per tile, the batch workspace (extra_mats: further [tile][n][G] matrices the caller needs per tile),
// the seeds dealt to tile slots (d_seeds, d_slot_k, d_evoff)
int resolve_G(const rwr_graph *g, int32_t K);
int32_t ensure_workspace(rwr_graph *g, int G, int32_t K, int *TG_out, int extra_mats = 0);
int32_t upload_seed_slots(rwr_graph *g, const int32_t *seeds, int32_t K, int G, std::vector<int32_t> *slot_k_out,
                          std::vector<int32_t> *slot_seed_out = nullptr);

}  // namespace rwr
