// Ranked walks within a caller-set candidate pool and with per-seed deny lists (rwr_recommend_filtered_batch,
// rwr_recommend_filtered_positions_batch).  The walk, the link exclusion and the destinations are the typed
// entries' (typed.hip's driver, ranked_end.h); what is this file's is the candidate list of ONE call: the rows of the wanted
// node type (or of any) that the caller's pool lists, compacted on the device from the pool's unsorted index list and dropped
// when the call ends -- the pool changes from call to call, so nothing is cached and the handle's per-type lists are left
// alone.  The deny lists need no kernel of their own: they are the ranked end's second set description, marked by
// k_exclude_members.
#include "filter.h"

namespace rwr {

// ---- the pool as a bitmap over the rows ----------------------------------------------------------------------------------------

// one pool entry per thread and trip: bit (i & 31) of word (i >> 5).  An index listed twice, or two indices of one word from
// different waves, meet in the atomic OR: the bitmap is the set of the listed rows whatever the order of the stores
__global__ __launch_bounds__(FILTER_MARK_BLOCK) void k_pool_mark(int32_t n, int64_t count, const int32_t *__restrict__ pool,
                                                                 uint32_t *__restrict__ bitmap)
{
    const int64_t stride = (int64_t)gridDim.x * FILTER_MARK_BLOCK;
    for (int64_t q = (int64_t)blockIdx.x * FILTER_MARK_BLOCK + threadIdx.x; q < count; q += stride) {
        const int32_t i = pool[q];
        if (i >= 0 && i < n) atomicOr(&bitmap[filter_word(i)], filter_bit(i));   // (typed_call_check lets rows of [0, n) through only)
    }
}

// ---- candidate rows of a call: the pool marked, then typed.hip's compaction over the bitmap (filter_plan.h) ------------------

int32_t filter_rows_build(rwr_graph *g, int32_t cand_type, int64_t pool_count, const int32_t *pool_idx, DevBuf<int32_t> &list,
                          int32_t *nrows, Profile &prof)
{
    hipStream_t s = g->stream;
    const int32_t n = g->n;
    const bool pooled = pool_count >= 0;
    const size_t words = filter_bitmap_words(n);
    DevBuf<int32_t> off, d_pool;
    DevBuf<uint32_t> bitmap;
    RWR_TRY(off.alloc((size_t)cand_blocks(n) + 1));
    if (pooled) RWR_TRY(bitmap.alloc(words));
    if (pool_count > 0) RWR_TRY(d_pool.alloc((size_t)pool_count));
    return idle_on_error(s, [&]() -> int32_t {
        hipEvent_t a; RWR_TRY(prof.record(a, s));
        if (pooled) RWR_HIP(hipMemsetAsync(bitmap.p, 0, (words ? words : 1) * sizeof(uint32_t), s));
        if (pool_count > 0) {
            RWR_HIP(hipMemcpyAsync(d_pool.p, pool_idx, (size_t)pool_count * sizeof(int32_t), hipMemcpyHostToDevice, s));
            hipLaunchKernelGGL(k_pool_mark, dim3((unsigned)filter_mark_blocks(pool_count)), dim3(FILTER_MARK_BLOCK), 0, s, n, pool_count,
                               d_pool.p, bitmap.p);
        }
        RWR_TRY(cand_compact(g, cand_type, pooled ? bitmap.p : nullptr, off.p, list, nrows));
        RWR_TRY(prof.end(prof.rank, a, s));
        RWR_HIP(hipStreamSynchronize(s));                        // (off, the pool and the bitmap go back to the block cache on return)
        return RWR_OK;
    });
}

}  // namespace rwr
