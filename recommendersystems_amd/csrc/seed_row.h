// Everything that writes the seeds' own rows in exact mode (internal).  A seed's row is an n-term sequential fp64 chain
// (Model.cs:78-99 for target == seed), done either by a fold -- seed_chain.hip: literally, at the dependent-add rate, beside a
// batch's SpMM -- or by the binade scan -- chain_scan.hip: in parallel and still bit for bit, what a single-seed call waits
// for.  The same scan sums checkConvergence's |differences|.  Who launches which, and on which stream, is the step's business
// (GroupIter::step, iterate.hip) and the plan's (step_plan.h).
#pragma once
#include "engine.h"
#include "step_plan.h"

namespace rwr {

// ---- seed_chain.hip: the folds --------------------------------------------------------------------------------------------
// k_seed_terms: the addends of the links into the seeds, into g->d_evterm at evoff[slot] (Zin != nullptr: value-free form, the
// z matrix holds them; nz: the frontier bitmap of X, when X may hold stale rows -- DESIGN §3.3.2)
void launch_seed_terms(rwr_graph *g, int G, int tg, const double *X, const int32_t *seeds, double c1, const int64_t *evoff,
                       hipStream_t s, const double *Zin, const uint32_t *nz = nullptr);
// The fold of kind Chain::Sparse (over the non-zero rows of the bitmap nz_x), Chain::Roles (masked: X holds stale rows outside
// nz_x) or the one-lane reference kernel; gate != nullptr: the fold's workgroups check in there
void launch_chain(rwr_graph *g, int G, int tg, const double *X, double *Y, const int32_t *seeds, double c1, const int64_t *evoff,
                  uint32_t *nz_out, unsigned int *gate, hipStream_t s, Chain kind, const uint32_t *nz_x, bool masked);
// k_gate: holds stream s until `expected` fold workgroups have checked in at *gate (or 1 ms has passed)
void launch_gate(const unsigned int *gate, unsigned int expected, hipStream_t s);

// ---- chain_scan.hip: the binade scan --------------------------------------------------------------------------------------
// once per tile group (the scan workspace and each block's share of the seeds' in-link lists), then once per step
int32_t chain_scan_prepare(rwr_graph *g, int G, int tg, const int32_t *d_seeds, hipStream_t s);
int32_t chain_scan_step(rwr_graph *g, int G, int tg, const double *X, double *Y, const int32_t *d_seeds,
                        const int64_t *d_evoff, double c1, uint32_t *nz_out, hipStream_t s, const double *zterms = nullptr,
                        double *zout = nullptr);
bool chain_scan_self_contained(int G);   // G == 1: no k_seed_terms / k_seed_z launches around the step
int32_t chain_scan_collect(rwr_graph *g, hipStream_t s);
int32_t chain_scan_sum(rwr_graph *g, const double *D, double *out, hipStream_t s);   // exact sequential sum of n addends >= 0
// ... of every column of a tile group's [tile][n][G] matrix of addends >= 0: sums[tile * G + k].  _prepare once per tile group
// (scratch cells and the all-zero link table; evoff: the group's d_evoff slots, never dereferenced past their pointer)
int32_t chain_scan_sum_cols_prepare(rwr_graph *g, int G, int tg, hipStream_t s);
int32_t chain_scan_sum_cols(rwr_graph *g, int G, int tg, const double *D, const int64_t *evoff, double *sums, hipStream_t s);

}  // namespace rwr
