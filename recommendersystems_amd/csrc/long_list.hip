// Ranked lists beyond the select's limit (long_list.h): top_n in (SEL_MAX_K, LONG_TOP_N_MAX] for
// rwr_recommend_long_batch and rwr_recommend_audience_set_long_batch.
//
// Per pass over some tiles of a group (long_plan.h: long_tiles_per_pass), after the exclusion, the deny marks and the cap:
//   1. the stock histogram / decide levels (rank_group_levels) for k = top_n: a segment's threshold is a prefix of the 128-bit
//      (score, id) key whose bin holds the k-th best entry and at most SEL_CAP members -- or all 128 bits, when more than
//      SEL_CAP candidates carry that very (score, id);
//   2. k_long_tie: only for such a spent segment, one workgroup walks the candidate list in order and finds the list position
//      of the k_rem-th member of the bin by ordered ballots.  The list is ascending in the row, so the members up to there are
//      the bin's k_rem smallest rows: exactly what the order (score desc, id desc, row asc) puts first;
//   3. k_long_collect: every candidate above the bin, and the bin's members (up to that position), take a slot of the segment
//      in a buffer of long_capacity(top_n) entries.  The slots are claimed by an integer atomic; WHICH entries are collected
//      is fixed by 1 and 2, there are never more than the capacity, and the order they arrive in is forgotten by the sort;
//   4. k_long_sort_runs: runs of LONG_RUN entries, one workgroup each, bitonic in LDS (rank_keys.h: sel_sort);
//   5. k_long_merge: long_passes(capacity) merge-path passes between the two buffers, one launch per pass for every segment
//      and every pair of runs; a thread finds its diagonal's split by binary search and writes LONG_MERGE_ITEMS outputs
//      (long_plan.h: long_pair_of, long_merge_range -- the host model runs the same functions).  The last pass stops at top_n;
//   6. k_long_emit: ids, scores, rows and counts in the tables' layout.
// Integer compares only: no floating-point atomic, no floating-point add.
#include "long_list.h"

#include "rank.h"
#include "rank_keys.h"

namespace rwr {

static_assert(LONG_SEL_MAX_K == SEL_MAX_K && LONG_SEL_CAP == SEL_CAP && LONG_SEL_LEVELS == SEL_LEVELS, "long_plan.h restates rank_keys.h");
static_assert(sizeof(LongKey) == sizeof(SelCandRow) && sizeof(LongKey) == 24, "the run sort's LDS: LONG_RUN x 24 bytes = 96 KiB of the CU's 160");
static_assert((2 * LONG_RUN) % LONG_MERGE_ITEMS == 0, "a thread's outputs lie inside one pair of runs");

// (sel_sort's order for the entries of this file)
__device__ __forceinline__ bool sel_lt(const LongKey &a, const LongKey &b) { return long_key_lt(a, b); }

constexpr int LONG_SORT_BLOCK = 1024, LONG_MERGE_BLOCK = 256;

// One workgroup per segment; only a segment whose levels spent all 128 bits has work.  tie[seg] = the list position of the
// k_rem-th candidate with exactly the threshold's (score, id), LONG_NO_TIE for every other segment
__global__ __launch_bounds__(256) void k_long_tie(int32_t n, int G, int32_t n_rows, const int32_t *__restrict__ rows,
                                                  const int64_t *__restrict__ node_id, const double *__restrict__ X,
                                                  const SelState *__restrict__ st, const int32_t *__restrict__ seeds,
                                                  int32_t *__restrict__ tie)
{
    __shared__ int wc[256 / WAVE];
    __shared__ int base_s, found_s;
    const int seg = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1), wv = tid / WAVE;
    const SelState my = st[seg];
    if (seeds[seg] < 0 || my.nbits != 128) {                    // (uniform)
        if (tid == 0) tie[seg] = LONG_NO_TIE;
        return;
    }
    const double *x = X + (size_t)(seg / G) * (size_t)n * G + (seg % G);
    if (tid == 0) base_s = 0, found_s = LONG_NO_TIE;
    __syncthreads();
    for (int32_t c0 = 0; c0 < n_rows; c0 += 256) {
        const int32_t q = c0 + tid;
        bool mem = false;
        if (q < n_rows) {
            const int32_t row = rows[q];
            const double s = x[(size_t)row * G];
            if (s >= 0.0) mem = f64_orderable(s) == my.ph && i64_orderable(node_id[row]) == my.pl;
        }
        const unsigned long long bal = __ballot(mem);
        if (lane == 0) wc[wv] = __popcll(bal);
        __syncthreads();
        int off = base_s;
        for (int w = 0; w < wv; ++w) off += wc[w];
        if (mem && off + (int)__popcll(bal & ((1ull << lane) - 1ull)) + 1 == my.k_rem) found_s = q;
        __syncthreads();
        if (tid == 0)
            for (int w = 0; w < 256 / WAVE; ++w) base_s += wc[w];
        __syncthreads();
        if (found_s != LONG_NO_TIE) break;                       // (uniform)
    }
    if (tid == 0) tie[seg] = found_s;
}

// explain.hip's k_sel_collect_rows with the segment's capacity and the bin's cut: a candidate at list position q goes in when
// it lies above the threshold's bin, or inside it at a position up to tie[segment]
template <int G>
__global__ __launch_bounds__(256) void k_long_collect(int32_t n, int32_t n_rows, const int32_t *__restrict__ rows,
                                                      const int64_t *__restrict__ node_id, const double *__restrict__ X,
                                                      SelState *__restrict__ st, const int32_t *__restrict__ seeds,
                                                      const int32_t *__restrict__ tie, int32_t cap, LongKey *__restrict__ cand)
{
    constexpr int RL = 256 / G;
    __shared__ SelState sst[G];
    __shared__ int32_t stie[G];
    const int tile = blockIdx.y;
    const int tid = threadIdx.x, k = tid % G, rl = tid / G;
    if (tid < G) sst[tid] = st[tile * G + tid], stie[tid] = tie[tile * G + tid];
    __syncthreads();
    if (seeds[tile * G + k] < 0) return;
    const SelState my = sst[k];
    const int32_t qt = stie[k];
    const double *x = X + (size_t)tile * (size_t)n * G;
    const int32_t q0 = blockIdx.x * SEL_ROWS_PER_BLOCK;
    const int32_t q1 = (q0 + SEL_ROWS_PER_BLOCK < n_rows) ? q0 + SEL_ROWS_PER_BLOCK : n_rows;
    for (int32_t q = q0 + rl; q < q1; q += RL) {
        const int32_t row = rows[q];
        const double s = x[(size_t)row * G + k];
        if (!(s >= 0.0)) continue;
        const uint64_t hi = f64_orderable(s);
        if (my.nbits > 0 && my.nbits <= 64 && (hi >> (64 - my.nbits)) < my.ph) continue;   // cheap reject
        const uint64_t lo = i64_orderable(node_id[row]);
        const int c = sel_cmp(hi, lo, my);
        if (c < 0 || (c == 0 && q > qt)) continue;
        const int slot = atomicAdd(&st[tile * G + k].cand_cnt, 1);
        if (slot < cap) cand[((size_t)tile * G + k) * (size_t)cap + slot] = LongKey{hi, lo, row, 0};
    }
}

// Workgroup (r, seg): run r of the segment's collected entries, sorted in place
__global__ __launch_bounds__(LONG_SORT_BLOCK) void k_long_sort_runs(const int32_t *__restrict__ slot_k, const SelState *__restrict__ st,
                                                                   int32_t cap, LongKey *__restrict__ cand)
{
    extern __shared__ LongKey lsc[];
    const int seg = blockIdx.y;
    if (slot_k[seg] < 0) return;
    int32_t cnt = st[seg].cand_cnt;
    if (cnt > cap) cnt = cap;
    const int32_t r0 = (int32_t)blockIdx.x * LONG_RUN;
    if (r0 >= cnt) return;
    const int len = cnt - r0 < LONG_RUN ? cnt - r0 : LONG_RUN;
    int N2 = 1;
    while (N2 < len) N2 <<= 1;
    LongKey *c = cand + (size_t)seg * (size_t)cap + r0;
    for (int i = threadIdx.x; i < N2; i += blockDim.x) lsc[i] = (i < len) ? c[i] : LongKey{0ull, 0ull, 0x7FFFFFFF, 0};
    __syncthreads();
    sel_sort(lsc, N2);
    for (int i = threadIdx.x; i < len; i += blockDim.x) c[i] = lsc[i];
}

// One merge pass over every segment: runs of `width` entries of src pairwise into dst.  limit_top_n > 0 (the last pass, one
// pair): outputs from there on are never read and not written
__global__ __launch_bounds__(LONG_MERGE_BLOCK) void k_long_merge(const int32_t *__restrict__ slot_k, const SelState *__restrict__ st,
                                                                int32_t cap, int64_t width, int32_t limit_top_n,
                                                                const LongKey *__restrict__ src, LongKey *__restrict__ dst)
{
    const int seg = blockIdx.y;
    if (slot_k[seg] < 0) return;
    int64_t cnt = st[seg].cand_cnt;
    if (cnt > cap) cnt = cap;
    const int64_t lim = (limit_top_n > 0 && limit_top_n < cnt) ? limit_top_n : cnt;
    const int64_t o = ((int64_t)blockIdx.x * LONG_MERGE_BLOCK + threadIdx.x) * LONG_MERGE_ITEMS;
    if (o >= lim) return;
    const LongPair pr = long_pair_of(o, width, cnt);
    const int64_t d = o - pr.base, left = pr.la + pr.lb - d;
    const LongKey *a = src + (size_t)seg * (size_t)cap + pr.base;
    long_merge_range(a, pr.la, a + pr.la, pr.lb, d, left < LONG_MERGE_ITEMS ? left : LONG_MERGE_ITEMS, dst + (size_t)seg * (size_t)cap + o);
}

// the first min(collected, top_n) entries of every live segment into row slot_k[seg] of the tables
__global__ __launch_bounds__(256) void k_long_emit(const int32_t *__restrict__ slot_k, const SelState *__restrict__ st, int32_t cap,
                                                   int32_t top_n, const LongKey *__restrict__ fin, int64_t *__restrict__ out_id,
                                                   double *__restrict__ out_score, int32_t *__restrict__ out_counts,
                                                   int32_t *__restrict__ out_row)
{
    const int seg = blockIdx.y;
    const int32_t orow = slot_k[seg];
    if (orow < 0) return;
    int32_t cnt = st[seg].cand_cnt;
    if (cnt > cap) cnt = cap;
    const int32_t take = cnt < top_n ? cnt : top_n;
    const int32_t i = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i == 0) out_counts[orow] = take;
    if (i >= take) return;
    const LongKey e = fin[(size_t)seg * (size_t)cap + i];
    const size_t cell = (size_t)orow * (size_t)top_n + (size_t)i;
    sel_decode(SelCand{e.hi, e.lo}, &out_id[cell], &out_score[cell]);
    out_row[cell] = e.row;
}

// ---- the host side ----------------------------------------------------------------------------------------------------------------

int32_t long_prepare(rwr_graph *g, LongEnd &l, int32_t K, int32_t top_n, hipStream_t s)
{
    const size_t cells = (size_t)K * (size_t)top_n;
    RWR_TRY(l.d_row.alloc(cells));
    RWR_HIP(hipMemsetAsync(l.d_row.p, 0xFF, cells * sizeof(int32_t), s));
    return RWR_OK;
}

// a buffer of the call that a later group needs larger: the stream is drained before the old block goes back to the cache
template <class T>
static int32_t grow_idle(DevBuf<T> &b, size_t elems, hipStream_t s)
{
    if (b.p && b.count >= elems) return RWR_OK;
    if (b.p) RWR_HIP(hipStreamSynchronize(s));
    return b.alloc(elems);
}

int32_t long_rank_group(rwr_graph *g, LongEnd &l, int G, int tg, const int32_t *slot_k, int32_t top_n, const double *X, hipStream_t s,
                        const int32_t *rows, int32_t nrows)
{
    if (!long_applies(top_n) || top_n > LONG_TOP_N_MAX) { set_error("long lists: top_n %d is outside the long path's range", top_n); return RWR_E_INVALID; }
    const int32_t cap = (int32_t)long_capacity(top_n), passes = long_passes(cap), runs = long_runs(cap);
    const int tc = long_tiles_per_pass(tg, G, top_n);
    RWR_HIP(hipFuncSetAttribute((const void *)k_long_sort_runs, hipFuncAttributeMaxDynamicSharedMemorySize,
                                LONG_RUN * (int)sizeof(LongKey)));   // (per launch: the attribute is per device)
    for (int t0 = 0; t0 < tg; t0 += tc) {
        const int tt = tg - t0 < tc ? tg - t0 : tc, nseg = tt * G;
        const int32_t *sk = slot_k + (size_t)t0 * G;
        const double *Xt = X + (size_t)t0 * (size_t)g->n * G;
        RWR_TRY(grow_idle(l.d_tie, (size_t)nseg, s));
        RWR_TRY(grow_idle(l.d_alt, (size_t)nseg * (size_t)cap * sizeof(LongKey), s));
        SelState *st = nullptr;
        void *cand_v = nullptr;
        RWR_TRY(rank_group_levels(g, G, tt, top_n, Xt, sk, s, rows, nrows, sizeof(LongKey), &st, &cand_v, (size_t)cap));
        LongKey *src = (LongKey *)cand_v, *dst = (LongKey *)l.d_alt.p;
        hipLaunchKernelGGL(k_long_tie, dim3((unsigned)nseg), dim3(256), 0, s, g->n, G, nrows, rows, g->node_id.p, Xt, st, sk, l.d_tie.p);
        const unsigned nblk = cdiv((size_t)nrows, SEL_ROWS_PER_BLOCK);
        RWR_DISPATCH_G(G, hipLaunchKernelGGL(k_long_collect<GG>, dim3(nblk, tt), dim3(256), 0, s, g->n, nrows, rows, g->node_id.p, Xt, st,
                                             sk, l.d_tie.p, cap, src));
        hipLaunchKernelGGL(k_long_sort_runs, dim3((unsigned)runs, (unsigned)nseg), dim3(LONG_SORT_BLOCK), LONG_RUN * sizeof(LongKey), s, sk,
                           st, cap, src);
        for (int32_t p = 0; p < passes; ++p) {
            const bool last = p == passes - 1;
            const size_t outs = last ? (size_t)top_n : (size_t)cap;
            hipLaunchKernelGGL(k_long_merge, dim3(cdiv(outs, (size_t)LONG_MERGE_BLOCK * LONG_MERGE_ITEMS), (unsigned)nseg),
                               dim3(LONG_MERGE_BLOCK), 0, s, sk, st, cap, long_pass_width(p), last ? top_n : 0, src, dst);
            LongKey *sw = src; src = dst; dst = sw;
        }
        hipLaunchKernelGGL(k_long_emit, dim3(cdiv((size_t)top_n, 256), (unsigned)nseg), dim3(256), 0, s, sk, st, cap, top_n, src,
                           g->d_out_id.p, g->d_out_score.p, g->d_counts.p, l.d_row.p);
        RWR_HIP(hipGetLastError());
    }
    return RWR_OK;
}

int32_t long_copy_back(rwr_graph *g, LongEnd &l, int32_t K, int32_t top_n)
{
    hipStream_t s = g->stream;
    if (l.nodes) RWR_HIP(hipMemcpyAsync(l.nodes, l.d_row.p, (size_t)K * (size_t)top_n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    RWR_HIP(hipStreamSynchronize(s));
    return RWR_OK;
}

}  // namespace rwr
