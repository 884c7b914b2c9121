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

// What the finishing workgroup of a slot (256 threads, all of them here) does first, for either destination: the slot's h + 1
// interval counters c become their inclusive prefix sums in place, 256 at a time behind a running carry; *carry (LDS) ends
// as their total, the slot's list length.  sh: 256 words of LDS.  Ends behind a barrier.
__device__ __forceinline__ void eval_prefix_counters(uint32_t *c, int32_t h, uint32_t *sh, uint32_t *carry)
{
    const int tid = threadIdx.x;
    if (tid == 0) *carry = 0;
    __syncthreads();
    for (int32_t base = 0; base <= h; base += 256) {
        const int32_t i = base + tid;
        sh[tid] = (i <= h) ? c[i] : 0u;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {
            const uint32_t t = tid >= off ? sh[tid - off] : 0u;
            __syncthreads();
            sh[tid] += t;
            __syncthreads();
        }
        if (i <= h) c[i] = *carry + sh[tid];
        __syncthreads();
        if (tid == 255) *carry += sh[255];
        __syncthreads();
    }
}

// What both destinations prepare: the plan of this slot assignment (slots_per_group slots form a tile group), its device copy
// and the scratch of one tile group.  out_a, out_b: the result arrays whose presence eval_check looks at.  The host vectors
// are pageable: the caller synchronises s.
int32_t eval_plan_upload(EvalEnd &ev, int32_t K, const std::vector<int32_t> &slot_k, size_t slots_per_group, const void *out_a,
                         const void *out_b, const char *who, hipStream_t s);
// ... and the zeroed result records of the Hits / AP destination
int32_t eval_prepare(rwr_graph *g, EvalEnd &ev, int32_t K, const std::vector<int32_t> &slot_k, size_t slots_per_group,
                     const char *who, hipStream_t s);
// A tile group (tg tiles of G slots from slot q0 on) holds its final ranks in X, the excluded elements at -1: hits, sort,
// count, finish over the candidate rows rows[0 .. nrows) (a device list: the ITEM rows, or those of another node type).
// g->d_slot_k holds the slots' batch positions.  Synchronises s once (the slots' hit counts).  nrows == 0: nothing is launched.
// eval_count_group is stages 1-3 (nrows > 0) for a destination that finishes by itself (eval_pos.hip): ev.layout, ev.d_hit_off,
// ev.d_sorted and ev.d_counters describe the group when it returns.
int32_t eval_count_group(rwr_graph *g, EvalEnd &ev, int G, int tg, size_t q0, const double *X, const int32_t *rows, int32_t nrows,
                         hipStream_t s);
int32_t eval_group(rwr_graph *g, EvalEnd &ev, int G, int tg, size_t q0, const double *X, const int32_t *rows, int32_t nrows,
                   hipStream_t s);
// after the last group: the K records into the caller's arrays (one copy, one synchronisation)
int32_t eval_copy_back(rwr_graph *g, EvalEnd &ev, int32_t K, const char *who, hipStream_t s);

}  // namespace rwr
