// What each step of a tile group's power iteration does, decided by plan_step() from the group's
// PlanConfig and the step number alone and carried out by GroupIter::step (iterate.hip).  Plain C++17 without HIP, so that
// tests/cpp/step_plan_check.cpp checks the rules on the host.
#pragma once

#include <cstdint>

namespace rwr {

// Per-link tile masks (§3.3.2): graphs of fewer links keep the per-entry bitmap probe (the measurements behind the figure: §3.3.2)
constexpr int64_t ENTRY_LIVE_MIN_NNZ = 100000000;

// What a group's plan depends on.  First the environment values (iterate.hip: plan_knobs; defaults: the shipped library's):
// RWR_SPMM (0: plain kernel, no bitmaps), RWR_NZ_ITERS, RWR_ACT_ITERS (-1: by graph shape), RWR_ACT_MIN_N, RWR_FRONTIER_LIST,
// RWR_CHAIN (0 simple, 1 auto, 2 scan, 3 role-specialised fold), RWR_SCAN_WORK, RWR_SCAN_SIDE, RWR_GATE, RWR_TAIL_ROWS,
// RWR_X_CLEAR (1: clear X on every fresh batch), RWR_ENTRY_LIVE (0: every probing step probes the bitmaps per entry and tile,
// 1: per-link tile masks where the graph is large enough, 2: wherever the rule's other conditions hold).
struct PlanInput {
    int spmm = 1, nz_iters = 4, act_iters = -1, frontier_list = 1, chain = 1, x_clear = 0;
    int64_t act_min_n = 200000; double scan_work = 10000.0;
    int scan_side = 1, gate = 1, tail_rows = 1;
    bool two_streams = true;      // a chain may run on the second stream (RWR_CHAIN_SERIAL=0)
    int32_t n = 0, big_n = 2000000;   // the graph: nodes, spmv_big_n(), links, weights >= 0 and finite
    int64_t nnz = 0; bool nonneg = true;
    int seed_row_kernel = 0;      // opts.seed_row_kernel: 1 fold, 2 scan, 3 simple; 0 = RWR_CHAIN
    bool scan_self = false;       // chain_scan_self_contained(G)
    int G = 1, tg = 1;            // seeds per tile, tiles in the group
    double c1 = 0.85;             // 1 - d
    bool fresh = true;            // Model ctor ranks; false: X holds caller-supplied ranks, whose frontier is unknown
    bool ranks_nonneg = true;     // the caller-supplied ranks are >= 0
    bool ranking_only = false;    // the caller reads only the ranking (recommend_batch): row-list steps allowed
    int entry_live = 1;           // RWR_ENTRY_LIVE
    int64_t entry_live_min_nnz = ENTRY_LIVE_MIN_NNZ;
};

// Everything fixed for one tile group
struct PlanConfig {
    int G = 1, tg = 1; bool fresh = true;
    int nz_iters = 0;             // steps 0 .. nz_iters - 1 probe the bitmap of X's non-zero rows (all but the last write the next)
    int act_iters = 0;            // steps 0 .. act_iters - 1 of those also mark the out-neighbours of those rows (act steps)
    bool flist = false;           // frontier-list steps allowed (§3.3.2): rows of X / Z outside the bitmaps may be stale
    bool addends_nonneg = false;  // weights, ranks and 1-d all >= 0 and finite: exact parallel reductions are allowed
    bool scan = false;            // the chain of a step that marks nothing is the binade scan; else chain_kind 0 the simple
    int chain_kind = 1;           // one-lane kernel, any other the role-specialised fold
    bool scan_side = false, scan_self = false;   // the scan runs on the second stream / gathers its terms from Z itself
    bool two_streams = true, gate = true;        // a fold runs on the second stream / the SpMM waits for its workgroups
    bool tails = false; int tail_depth = 0;   // the last steps may walk the tail row lists of this many levels (§3.3.1)
    unsigned need = 0;            // bit k: some seed of the group needs its chain at step T - 1 - k (the OR of h_tail_flag)
    bool force_clear = false;     // RWR_X_CLEAR=1
    bool clear_x = true;          // a fresh batch clears X before its seeds are written (plan_clear_x)
    bool entry_live = false;      // the probing steps that walk every row read per-link tile masks (§3.3.2, plan_entry_live)
};

// Whether a fresh batch must clear X (§3.3.2).  A frontier-list step writes only its listed rows, and the chain of the step
// after it may read every row (plan_step: chain_masked).  Without the clear the unlisted rows are stale, and that chain must
// read through the bitmap the list step wrote: only the role-specialised fold has such a form.  The scan and the simple fold
// keep the clear, and so does every group that never lists.  To be called again whenever flist changes.
inline bool plan_clear_x(const PlanConfig &c) { return c.force_clear || !c.flist || c.scan || c.chain_kind == 0; }

// Whether a group's probing steps may read per-link tile masks instead of probing the frontier bitmaps per entry and tile:
// only recommend_batch's groups (fresh ranks, ranking only) on the chunked kernels, with bitmaps at all, and -- unless
// RWR_ENTRY_LIVE=2 -- on a graph whose pass over all links pays.  GroupIter::init withdraws it when the masks get no memory.
inline bool plan_entry_live(const PlanInput &in, const PlanConfig &c)
{
    if (in.entry_live == 0 || !in.ranking_only || !in.fresh || in.G < 8 || c.nz_iters <= 0) return false;
    return in.entry_live == 2 || in.nnz >= in.entry_live_min_nnz;
}

inline PlanConfig plan_config(const PlanInput &in)
{
    PlanConfig c;
    c.G = in.G, c.tg = in.tg, c.fresh = in.fresh;
    const bool single = in.G == 1 && in.tg == 1;   // one seed: the lane-per-row SpMV
    // (skipping +0.0 addends is only a bitwise no-op while every accumulator is >= +0.0: weights must be >= 0)
    c.nz_iters = (in.G >= 8 && in.spmm != 0 && in.nonneg) ? in.nz_iters : 0;
    // steps 0 and 1 mark the out-neighbours of the few non-zero rows (step 1 only on sparse graphs: on dense ones --
    // hundreds of links per node -- marking the 2-hop neighbourhood costs more atomics than the skipped rows save)
    c.act_iters = in.act_iters >= 0 ? in.act_iters : ((in.nnz / (in.n > 0 ? in.n : 1)) <= 64 ? 2 : 1);
    // single seed: row-level skipping only, for exactly those steps; a third on a multi-million-node sparse graph (-7 % per
    // call on the 6 M-node graph, +10 % on the 0.6 M-node one), none below act_min_n (marking 38 us, dense step 8, at 12 K)
    if (single && in.act_iters < 0 && c.act_iters == 2 && in.n >= in.big_n) c.act_iters = 3;
    if (single && in.spmm != 0 && in.nonneg) c.nz_iters = c.act_iters;
    if (single && in.act_iters < 0 && in.n < in.act_min_n) c.nz_iters = c.act_iters = 0;
    if (!in.fresh) c.nz_iters = c.act_iters = 0;
    // a frontier-list step needs a bitmap-probing step after it (nz_iters >= 2) and a per-tile row list
    c.flist = in.ranking_only && in.fresh && in.frontier_list != 0 && in.G >= 8 && c.nz_iters >= 2 && c.act_iters >= 1;
    // The fold takes ~10 ns per node and step whatever the batch (hidden behind a large batch's SpMM); the scan is parallel,
    // ~6.7 ps per (node, seed) on top of an SpMM of ~0.89 ps per (link, seed) (measured, MI355X, 20 M- and 200 M-link
    // graphs) => auto takes the scan while  seeds * (0.89 * links/node + 6.7) < 10000.
    c.chain_kind = in.seed_row_kernel == 1 ? 3 : in.seed_row_kernel == 2 ? 2 : in.seed_row_kernel == 3 ? 0 : in.chain;
    const double per_seed = 0.89 * (double)in.nnz / (double)(in.n > 0 ? in.n : 1) + 6.7;
    c.addends_nonneg = in.c1 >= 0.0 && in.c1 <= 1.0 && in.nonneg && in.ranks_nonneg;
    c.scan = c.addends_nonneg && (c.chain_kind == 2 || (c.chain_kind == 1 && (double)in.tg * in.G * per_seed < in.scan_work));
    // a single seed's scan beside its SpMV, only where the kernels outlast the fork / join (-29 % at 224 K nodes, +19 % at 12 K)
    c.scan_side = in.scan_side != 0 && single && in.two_streams && in.n >= 100000;
    c.scan_self = in.scan_self, c.two_streams = in.two_streams, c.gate = in.gate != 0;
    c.tails = in.ranking_only && in.tail_rows != 0 && !single;   // (a single seed's SpMV walks every row)
    c.force_clear = in.x_clear != 0;
    c.clear_x = plan_clear_x(c);
    c.entry_live = plan_entry_live(in, c);
    return c;
}

// The rows a step's SpMM walks: every row (row_order), the tile's frontier list (fl_rows) or tail level k (tail_rows[k])
enum class Rows : uint8_t { All, Frontier, Tail };
struct RowSource { Rows kind = Rows::All; int level = 0; };
// The seed-row chain: none, the binade scan (main / second stream), the bitmap-walking sparse fold (act steps), the
// role-specialised fold or the simple one-lane fold
enum class Chain : uint8_t { None, Scan, ScanSide, Sparse, Roles, Simple };

struct StepPlan {
    RowSource rows;
    bool probe = false, write_bits = false;   // the SpMM reads through the current frontier bitmap / writes the next one
    bool mark = false;                        // k_mark_active marks the rows the step can reach (an act step)
    bool terms_nz = false;                    // k_seed_terms reads through the current bitmap (rows outside it may be stale)
    Chain chain = Chain::None;
    bool chain_masked = false;                // the chain reads X through the current bitmap: rows outside it are stale (!clear_x)
    bool chain_side = false, gate = false;    // the chain runs on the second stream / the SpMM waits for it (k_gate)
    bool chain_self = false;                  // the scan gathers its terms from Z and forms the seed rows' next z
    bool form_z = false, seed_z = false;      // value-free path: the SpMM / k_seed_z forms the next z
    bool entry_live = false;                  // the SpMM reads the step's per-link tile masks instead of probing (k_entry_live)
    bool dense() const { return !probe && rows.kind == Rows::All; }
    bool scan() const { return chain == Chain::Scan || chain == Chain::ScanSide; }
};

// The tail plan (§3.3.1): step T - 1 - k walks tail_rows[k] for k <= last_tail() (-1: none) and runs its chain only with
// need bit k.  The first step whose chain runs is the last restricted one: that chain reads every row of the step before,
// which therefore stays whole.  Without a need bit below the depth, the last tail_depth steps are restricted and chainless.
inline int last_tail(const PlanConfig &c)
{
    for (int k = 0; c.tails && k < c.tail_depth; ++k)
        if ((c.need >> k) & 1u) return k;
    return c.tails ? c.tail_depth - 1 : -1;
}

// Whether step `it` of T walks its tile's frontier list.  A frontier-list step writes only its frontier's rows of Y / Z.
// Allowed where the next step reads the output only through the bitmap this step writes: it probes it and either is itself an
// act step (bitmap-walking chain) or, at it = 1, writes over X_0, whose only non-zero rows -- the seed rows -- are listed: its
// output is whole where X_0 was cleared, and is read through the bitmap where it was not (chain_masked).  Tail steps, the
// last step and a run that may stop after any step never list.
inline bool step_lists(const PlanConfig &c, int64_t it, int64_t T)
{
    const int64_t k = T - 1 - it;
    if (!c.flist || T < 0 || it < 0 || k <= 0 || k <= last_tail(c)) return false;
    const bool write_bits = it + 1 < c.nz_iters, mark = it < c.nz_iters && it < c.act_iters;
    return mark && write_bits && (it + 1 < c.act_iters || it == 1);
}

// Step `it` of T (T < 0: a run whose end is not known in advance -- no step is the last and none walks a row list)
inline StepPlan plan_step(const PlanConfig &c, int64_t it, int64_t T)
{
    StepPlan p;
    const int64_t k = T - 1 - it;   // (T >= 0) steps still to come: 0 = the last step
    const bool last = T >= 0 && k == 0, tail = T >= 0 && k <= last_tail(c);
    p.probe = it < c.nz_iters;
    p.write_bits = it + 1 < c.nz_iters;
    p.mark = p.probe && it < c.act_iters;
    p.terms_nz = c.flist && p.probe;
    if (tail)
        p.rows = {Rows::Tail, (int)k};
    else if (step_lists(c, it, T))
        p.rows = {Rows::Frontier, 0};
    // (while X is sparse the bitmap-walking chain serves a whole tile at once; for a single seed the scan is cheaper)
    if (tail && !((c.need >> k) & 1u)) p.chain = Chain::None;
    else if (c.scan && (!p.mark || c.G == 1)) p.chain = c.scan_side ? Chain::ScanSide : Chain::Scan;
    else if (p.mark) p.chain = Chain::Sparse;
    else p.chain = c.chain_kind == 0 ? Chain::Simple : Chain::Roles;
    // a chain that reads every row of a frontier-list step's output (the bitmap-walking one reads the listed rows only)
    p.chain_masked = !c.clear_x && p.chain != Chain::None && p.chain != Chain::Sparse && step_lists(c, it - 1, T);
    const bool fold = p.chain != Chain::None && !p.scan();
    p.chain_side = p.chain == Chain::ScanSide || (fold && c.two_streams);
    p.gate = fold && c.two_streams && c.gate;
    p.chain_self = p.scan() && c.scan_self;
    p.form_z = !last;
    p.seed_z = p.form_z && p.chain != Chain::None && !p.chain_self;
    // a frontier list or a tail list visits too few links to pay for a pass over all of them
    p.entry_live = c.entry_live && c.G >= 8 && p.probe && p.rows.kind == Rows::All;
    return p;
}

}  // namespace rwr
