// The positions destination of a ranked end (internal; eval_pos.hip): the position and score of every test id in
// its slot's whole list, by the counting evaluation's stages 1-3 (eval_count.h) and a finish of its own.
#pragma once
#include "eval_count.h"
#include "pos_plan.h"

namespace rwr {

// A RankedEnd's third destination (ranked_end.h, whose lifetime rule it shares): the caller's arrays, the plan of the scatter
// back into them, and the device result arrays parallel to ev.plan.ids.  ev carries the test sets and the scratch of stages
// 1-3; its Hits / AP fields stay unused.
struct PosEnd {
    EvalEnd ev;
    int64_t *pos_out = nullptr;        // [test_ptr[K]]
    double *score_out = nullptr;       // [test_ptr[K]], may be NULL
    int64_t *list_len = nullptr;       // [K], may be NULL
    PosPlan plan;
    DevBuf<int64_t> d_pos;             // [ids] -1, then the smallest position of a hit carrying the id
    DevBuf<double> d_score;            // [ids] +0.0, then that hit's score
    DevBuf<int64_t> d_len;             // [K] 0, then the list length at the vector's batch position
};

// the plans of this slot assignment, their device copies, the result arrays at -1 / +0.0 / 0.  The host vectors are pageable:
// the caller synchronises s.
int32_t pos_prepare(rwr_graph *g, PosEnd &pe, int32_t K, const std::vector<int32_t> &slot_k, size_t slots_per_group,
                    const char *who, hipStream_t s);
// a tile group as eval_group takes it: hits, sort, count, then every hit's position into its id's place
int32_t pos_group(rwr_graph *g, PosEnd &pe, int G, int tg, size_t q0, const double *X, const int32_t *rows, int32_t nrows,
                  hipStream_t s);
// after the last group: one copy of the result arrays, then the scatter into the caller's order on the host
int32_t pos_copy_back(rwr_graph *g, PosEnd &pe, int32_t K, const char *who, hipStream_t s);

}  // namespace rwr
