// What the two files of the graph build share: build.hip (all device code, the general multi-launch build) and build_small.hip
// (the host side of the one-launch build of ego-network-sized graphs).
#pragma once
#include "engine.h"

namespace rwr {

// the experiments build's wall-clock stamps of the build's stages (RWR_BUILD_TIMING=1; engine.h: Stamps)
static const Stamps build_stamps("build", "RWR_BUILD_TIMING");

// build.hip
int32_t graph_build_upload(rwr_graph *g, const int64_t *node_id, const uint8_t *node_type, const int64_t *rowptr,
                           const int32_t *dst, const uint8_t *etype, const double *w);
int row_order_mode();   // RWR_ROW_ORDER (experiments build): 0 = in-degree descending, what the library ships
// the link count and the build's flag words ([0] some row non-uniform, [1] bad target, [2] max in-degree, [3] a weight or row
// sum not in (0, inf)) applied to the handle: nnz, uniform, nonneg, vf; a bad target is the build's one data error
int32_t graph_apply_flags(rwr_graph *g, int64_t nnz, const int *h_flags);
// host side of a finished build (h_in_ptr read back): bins of the in-degree orders, statistics
int32_t derive_finish(rwr_graph *g, const int *h_flags, hipEvent_t e0, hipEvent_t e1);
// k_build_small for one graph, k_build_small_multi for a device array of `count` argument blocks (one workgroup each)
int32_t launch_build_small(const BuildSmallArgs &a, hipStream_t s);
int32_t launch_build_small_multi(const BuildSmallArgs *d_args, int32_t count, hipStream_t s);
#ifdef RWR_EXPERIMENTS
void row_pass_stamps(unsigned long long out[16]);   // s_memrealtime stamps of the row pass of rows 0..63 (RP_STAMP)
#endif

// build_small.hip
bool small_build_ok(const rwr_graph *g);
int32_t graph_derive_small(rwr_graph *g, bool first);

}  // namespace rwr
