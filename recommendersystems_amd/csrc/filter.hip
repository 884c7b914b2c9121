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
        if (i >= 0 && i < n) atomicOr(&bitmap[filter_word(i)], filter_bit(i));   // (filter_check lets rows of [0, n) through only)
    }
}

// ---- candidate rows of a call: count per block, scan of the counts, ordered scatter (typed.hip's k_cand_*, filter_plan.h) -----

// does this thread's row match, and the wave's matches as a ballot; wc[w] = matches of wave w of the workgroup
__device__ __forceinline__ bool filter_row_match(int32_t n, const uint8_t *__restrict__ node_type, int32_t t,
                                                 const uint32_t *__restrict__ bitmap, int32_t *wc, unsigned long long *bal)
{
    const int32_t b = blockIdx.x;
    const int32_t i = cand_block_lo(b) + (int32_t)threadIdx.x;
    const bool m = i < cand_block_hi(b, n) && filter_match(node_type, t, bitmap, i);
    *bal = __ballot(m);
    if ((threadIdx.x & (WAVE - 1)) == 0) wc[threadIdx.x / WAVE] = __popcll(*bal);
    __syncthreads();
    return m;
}

__global__ __launch_bounds__(CAND_BLOCK) void k_filter_count(int32_t n, const uint8_t *__restrict__ node_type, int32_t t,
                                                             const uint32_t *__restrict__ bitmap, int32_t *__restrict__ block_cnt)
{
    __shared__ int32_t wc[CAND_BLOCK / WAVE];
    unsigned long long bal;
    filter_row_match(n, node_type, t, bitmap, wc, &bal);
    if (threadIdx.x == 0) {
        int32_t c = 0;
        for (int w = 0; w < CAND_BLOCK / WAVE; ++w) c += wc[w];
        block_cnt[blockIdx.x] = c;
    }
}

__global__ __launch_bounds__(CAND_BLOCK) void k_filter_scatter(int32_t n, const uint8_t *__restrict__ node_type, int32_t t,
                                                               const uint32_t *__restrict__ bitmap, const int32_t *__restrict__ off,
                                                               int32_t total, int32_t *__restrict__ rows)
{
    __shared__ int32_t wc[CAND_BLOCK / WAVE];
    unsigned long long bal;
    if (!filter_row_match(n, node_type, t, bitmap, wc, &bal)) return;
    const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
    int32_t pos = off[blockIdx.x];
    for (int q = 0; q < wv; ++q) pos += wc[q];
    pos += __popcll(bal & ((1ull << lane) - 1ull));
    if (pos >= 0 && pos < total) rows[pos] = cand_block_lo(blockIdx.x) + (int32_t)threadIdx.x;
}

int32_t filter_rows_build(rwr_graph *g, int32_t cand_type, int64_t pool_count, const int32_t *pool_idx, DevBuf<int32_t> &list,
                          int32_t *nrows, Profile &prof)
{
    hipStream_t s = g->stream;
    const int32_t n = g->n, nb = cand_blocks(n);
    const bool pooled = pool_count >= 0;
    const size_t words = filter_bitmap_words(n);
    DevBuf<int32_t> off, d_pool;
    DevBuf<uint32_t> bitmap;
    RWR_TRY(off.alloc((size_t)nb + 1));
    if (pooled) RWR_TRY(bitmap.alloc(words));
    if (pool_count > 0) RWR_TRY(d_pool.alloc((size_t)pool_count));
    int32_t total = 0;
    RWR_TRY(idle_on_error(s, [&]() -> int32_t {
        hipEvent_t a; RWR_TRY(prof.record(a, s));
        if (pooled) RWR_HIP(hipMemsetAsync(bitmap.p, 0, (words ? words : 1) * sizeof(uint32_t), s));
        if (pool_count > 0) {
            RWR_HIP(hipMemcpyAsync(d_pool.p, pool_idx, (size_t)pool_count * sizeof(int32_t), hipMemcpyHostToDevice, s));
            hipLaunchKernelGGL(k_pool_mark, dim3((unsigned)filter_mark_blocks(pool_count)), dim3(FILTER_MARK_BLOCK), 0, s, n, pool_count,
                               d_pool.p, bitmap.p);
        }
        const uint32_t *bm = pooled ? bitmap.p : nullptr;
        if (nb > 0) hipLaunchKernelGGL(k_filter_count, dim3((unsigned)nb), dim3(CAND_BLOCK), 0, s, n, g->node_type.p, cand_type, bm, off.p);
        launch_cand_scan(nb, off.p, s);
        RWR_HIP(hipGetLastError());
        RWR_HIP(hipMemcpyAsync(&total, off.p + nb, sizeof(int32_t), hipMemcpyDeviceToHost, s));
        RWR_HIP(hipStreamSynchronize(s));
        if (total < 0 || total > n) { set_error("candidate list build: %d rows of %d", total, n); return RWR_E_HIP; }
        RWR_TRY(list.alloc((size_t)total));
        if (total > 0)
            hipLaunchKernelGGL(k_filter_scatter, dim3((unsigned)nb), dim3(CAND_BLOCK), 0, s, n, g->node_type.p, cand_type, bm, off.p, total,
                               list.p);
        RWR_HIP(hipGetLastError());
        RWR_TRY(prof.end(prof.rank, a, s));
        RWR_HIP(hipStreamSynchronize(s));                        // (off, the pool and the bitmap go back to the block cache on return)
        return RWR_OK;
    }));
    *nrows = total;
    return RWR_OK;
}

// ---- the entries ----------------------------------------------------------------------------------------------------------------

int32_t recommend_filtered_batch(rwr_graph *g, const int32_t *seeds, int32_t K, double d, int32_t n_iter, int32_t top_n,
                                 int32_t cand_type, uint32_t excl_edge_mask, int32_t exclude_self, int64_t pool_count,
                                 const int32_t *pool_idx, const int64_t *deny_ptr, const int32_t *deny_idx, int64_t *ids,
                                 double *scores, int32_t *counts)
{
    CallFilter flt;
    flt.pool_count = pool_count, flt.pool_idx = pool_idx, flt.deny_ptr = deny_ptr, flt.deny_idx = deny_idx;
    RankedEnd end;
    end.who = "rwr_recommend_filtered_batch";
    end.top_n = top_n, end.ids = ids, end.scores = scores, end.counts = counts;
    return no_throw(end.who, [&] { return typed_body(g, seeds, K, d, n_iter, cand_type, excl_edge_mask, exclude_self, end, &flt); });
}

int32_t recommend_filtered_positions_batch(rwr_graph *g, const int32_t *seeds, int32_t K, double d, int32_t n_iter, int32_t cand_type,
                                           uint32_t excl_edge_mask, int32_t exclude_self, int64_t pool_count, const int32_t *pool_idx,
                                           const int64_t *deny_ptr, const int32_t *deny_idx, const int64_t *test_ptr,
                                           const int64_t *test_ids, int64_t *pos_out, double *score_out, int64_t *list_len)
{
    CallFilter flt;
    flt.pool_count = pool_count, flt.pool_idx = pool_idx, flt.deny_ptr = deny_ptr, flt.deny_idx = deny_idx;
    PosEnd pe;
    pe.ev.test_ptr = test_ptr, pe.ev.test_ids = test_ids;
    pe.pos_out = pos_out, pe.score_out = score_out, pe.list_len = list_len;
    RankedEnd end;
    end.who = "rwr_recommend_filtered_positions_batch";
    end.pos = &pe;
    return no_throw(end.who, [&] { return typed_body(g, seeds, K, d, n_iter, cand_type, excl_edge_mask, exclude_self, end, &flt); });
}

}  // namespace rwr
