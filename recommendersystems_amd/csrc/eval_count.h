// The counting evaluation of a tile group (internal; eval_count.hip): Hits / average precision of every slot's
// walk against its test set without a ranked list -- the position of a hit is the number of candidates that rank before it.
#pragma once
#include "engine.h"
#include "eval_plan.h"

namespace rwr {

// the record a slot's finishing workgroup writes at its vector's batch position, and the call copies back once
struct EvalOut {
    int64_t n_hits;
    double sum_precision;
    int64_t list_len;
};

// The evaluating destination of a RankedEnd (ranked_end.h, whose lifetime rule it shares): the caller's test sets and result
// arrays, the host plan, its device copy and the per-group scratch.
struct EvalEnd {
    const int64_t *test_ptr = nullptr, *test_ids = nullptr;
    int32_t top_n = 0;                 // > 0: Hits@N / AP@N; <= 0: the whole list
    int64_t *n_hits = nullptr;
    double *sum_precision = nullptr;
    int64_t *list_len = nullptr;       // may be NULL
    EvalPlan plan;
    DevBuf<int64_t> d_ids, d_slot_off; // the plan's sets and offsets
    DevBuf<EvalOut> d_out;             // [K], zeroed
    DevBuf<int32_t> d_flag;            // != 0: a hit list did not hold its hits (cannot happen: the lists are sized by a count)
    // one tile group at a time (the host vectors stay until the next synchronisation of the stream)
    std::vector<int32_t> h_cnt;
    EvalGroupLayout layout;
    DevBuf<int32_t> d_cnt, d_cursor;   // [group slots] hits counted / appended
    DevBuf<int64_t> d_hit_off;         // [group slots + 1]
    DevBuf<uint8_t> d_tile_lds;        // [tiles of the group]
    DevBuf<uint8_t> d_hits, d_sorted;  // the slots' hit keys (SelCand) as they arrive / descending
    DevBuf<uint32_t> d_counters;       // hits + 1 interval counters per slot
    DevBuf<double> d_terms;            // per hit (double)h / (pos + 1), in rank order
};

// the plan of this slot assignment (slots_per_group slots form a tile group) and its device copy; the zeroed result records.
// The host vectors are pageable: the caller synchronises s.
int32_t eval_prepare(rwr_graph *g, EvalEnd &ev, int32_t K, const std::vector<int32_t> &slot_k, size_t slots_per_group,
                     const char *who, hipStream_t s);
// A tile group (tg tiles of G slots from slot q0 on) holds its final ranks in X, the excluded elements at -1: hits, sort,
// count, finish over the candidate rows rows[0 .. nrows) (a device list: the ITEM rows, or those of another node type).
// g->d_slot_k holds the slots' batch positions.  Synchronises s once (the slots' hit counts).
int32_t eval_group(rwr_graph *g, EvalEnd &ev, int G, int tg, size_t q0, const double *X, const int32_t *rows, int32_t nrows,
                   hipStream_t s);
// after the last group: the K records into the caller's arrays (one copy, one synchronisation)
int32_t eval_copy_back(rwr_graph *g, EvalEnd &ev, int32_t K, const char *who, hipStream_t s);

}  // namespace rwr
