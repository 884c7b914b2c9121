// "Why is this entry here?" (rwr_recommend_explained_batch): the capped entry's lists with, per entry, its node
// index, its largest in-link addends and the number of positive ones.
//
// A list entry's score is the in-order sum of the addends fl(fl((1 - d) x_{T-1}[u]) * w(u -> v)) over v's in-list
// (Model.cs:84-87), and the typed driver still holds x_{T-1} when the list is written: GroupIter's Y after the last step
// (iterate.h), every row of it whole (the driver's plan is not ranking_only: step_plan.h allows row lists to nobody else).
// Two stages, both after the exclusion, the deny marks and the cap:
//   1. the ranking keeps the rows: after the stock histogram / decide levels (rank_group_levels) a collect and a
//      sort-and-emit of their own carry (score bits, id bits, row) and order by (score desc, id desc, row asc) -- a total
//      order, so the lists and the rows are the same on every run whatever the collect's append order was;
//   2. one workgroup per live (slot, entry) walks the entry's in-list: the lanes stride it, gather Y at their column, form the
//      addend and keep their best n_why keys (value bits, in-list position) in registers -- explain_plan.h's WhyList, the
//      model the host check runs as it stands; the lists are merged lane to lane by shuffles, wave to wave through LDS.
//      Integer compares and integer sums only: no atomic, no float add.
// Value-free graphs have no in_w: the weight of every link of source u is w_src[u], the same double.
#include "explain.h"

#include "rank_keys.h"
#include "ranked_end.h"

namespace rwr {

static_assert(WHY_MAX == RWR_WHY_MAX, "explain_plan.h's list and the header's limit");
static_assert(sizeof(SelCandRow) == 24, "the sort's LDS: SEL_SLOTS x 24 bytes = 96 KiB of the CU's 160");

// ---- 1. the row-carrying end of the select ---------------------------------------------------------------------------------------

// rank.hip's k_sel_collect with the row kept: every candidate at or above its segment's threshold takes a slot of the segment
template <int G>
__global__ __launch_bounds__(256) void k_sel_collect_rows(int32_t n, int32_t n_rows, const int32_t *__restrict__ rows,
                                                          const int64_t *__restrict__ node_id, const double *__restrict__ X,
                                                          SelState *__restrict__ st, const int32_t *__restrict__ seeds,
                                                          SelCandRow *__restrict__ cand)
{
    constexpr int RL = 256 / G;
    __shared__ SelState sst[G];
    const int tile = blockIdx.y;
    const int tid = threadIdx.x, k = tid % G, rl = tid / G;
    if (tid < G) sst[tid] = st[tile * G + tid];
    __syncthreads();
    if (seeds[tile * G + k] < 0) return;
    const SelState my = sst[k];
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
        if (sel_cmp(hi, lo, my) < 0) continue;
        const int slot = atomicAdd(&st[tile * G + k].cand_cnt, 1);
        if (slot < SEL_SLOTS) cand[((size_t)tile * G + k) * SEL_SLOTS + slot] = SelCandRow{hi, lo, row, 0};
    }
}

// one block per segment: bitonic sort by (score desc, id desc, row asc), the first top_n go out with their rows
__global__ __launch_bounds__(256) void k_sel_sort_emit_rows(const int32_t *__restrict__ slot_k, int32_t top_n,
                                                            const SelState *__restrict__ st, const SelCandRow *__restrict__ cand,
                                                            int64_t *__restrict__ out_id, double *__restrict__ out_score,
                                                            int32_t *__restrict__ out_counts, int32_t *__restrict__ out_row)
{
    extern __shared__ SelCandRow scr[];
    const int seg = blockIdx.x;
    const int32_t orow = slot_k[seg];            // batch position of this slot's seed
    if (orow < 0) return;
    int cnt = st[seg].cand_cnt;
    if (cnt > SEL_SLOTS) cnt = SEL_SLOTS;
    int N2 = 1;
    while (N2 < cnt) N2 <<= 1;
    const SelCandRow *c = cand + (size_t)seg * SEL_SLOTS;
    for (int i = threadIdx.x; i < N2; i += blockDim.x) scr[i] = (i < cnt) ? c[i] : SelCandRow{0ull, 0ull, 0x7FFFFFFF, 0};
    __syncthreads();
    sel_sort(scr, N2);
    const int take = cnt < top_n ? cnt : top_n;
    if (threadIdx.x == 0) out_counts[orow] = take;
    for (int i = threadIdx.x; i < take; i += blockDim.x) {
        const size_t cell = (size_t)orow * top_n + i;
        sel_decode(SelCand{scr[i].hi, scr[i].lo}, &out_id[cell], &out_score[cell]);
        out_row[cell] = scr[i].row;
    }
}

// ---- 2. the reasons ---------------------------------------------------------------------------------------------------------------

constexpr int WHY_BLOCK = 256, WHY_WAVES = WHY_BLOCK / WAVE;

// Workgroup (j, q): entry j of the list of slot q of the group.  in_w == nullptr: the value-free graph's weights, w_src[u].
// d_total == nullptr: no counts wanted; n_why == 0: counts only.
__global__ __launch_bounds__(WHY_BLOCK) void k_why(int32_t n, int G, int32_t top_n, int32_t n_why, double c1,
                                                   const int32_t *__restrict__ slot_k, const int32_t *__restrict__ counts,
                                                   const int32_t *__restrict__ out_row, const double *__restrict__ Y,
                                                   const int64_t *__restrict__ in_ptr, const int32_t *__restrict__ in_src,
                                                   const double *__restrict__ in_w, const double *__restrict__ w_src,
                                                   int32_t *__restrict__ d_src, double *__restrict__ d_term, int64_t *__restrict__ d_total)
{
    __shared__ WhyList sh_list[WHY_WAVES];
    __shared__ int64_t sh_cnt[WHY_WAVES];
    const int j = blockIdx.x, q = blockIdx.y;
    const int32_t orow = slot_k[q];
    if (orow < 0 || j >= counts[orow]) return;                   // (uniform: a padding slot, a cell behind the list)
    const size_t cell = (size_t)orow * (size_t)top_n + (size_t)j;
    const int32_t v = out_row[cell];
    if (v < 0 || v >= n) return;
    const int64_t p0 = in_ptr[v], deg = in_ptr[v + 1] - p0;
    if (deg <= 0) return;                                        // (the tables' unused state stands)
    const double *y = Y + (size_t)(q / G) * (size_t)n * G + (q % G);
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wv = tid / WAVE;

    WhyList l;
    why_list_init(l, n_why);
    int64_t cnt = 0;
    for (int64_t e = tid; e < deg; e += WHY_BLOCK) {
        const int32_t u = in_src[p0 + e];
        const double w = in_w ? in_w[p0 + e] : w_src[u];
        const double a = why_addend(c1, y[(size_t)u * G], w);
        if (!why_is_reason(a)) continue;
        ++cnt;
        why_list_insert(l, WhyKey{why_bits(a), (uint32_t)e});
    }
    // lane to lane: lane 0 of the wave ends with the wave's list (a stage whose partners all lie behind the in-list's end
    // has nothing to bring: deg is uniform)
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) {
        if ((int64_t)o >= deg) continue;
        WhyList other;
#pragma unroll
        for (int i = 0; i < WHY_MAX; ++i) {
            other.k[i].bits = __shfl_down((unsigned long long)l.k[i].bits, o);
            other.k[i].pos = __shfl_down(l.k[i].pos, o);
        }
        const long long oc = __shfl_down((long long)cnt, o);
        if (lane + o < WAVE) {
            why_list_merge(l, other);
            cnt += oc;
        }
    }
    // wave to wave
    const int nw = deg > (int64_t)(WHY_WAVES - 1) * WAVE ? WHY_WAVES : (int)((deg + WAVE - 1) / WAVE);   // waves with entries
    if (nw > 1) {
        if (lane == 0) sh_list[wv] = l, sh_cnt[wv] = cnt;
        __syncthreads();
    }
    if (tid != 0) return;
    for (int w = 1; w < nw; ++w) {
        const WhyList other = sh_list[w];
        why_list_merge(l, other);
        cnt += sh_cnt[w];
    }
    if (d_total) d_total[cell] = cnt;
    const size_t base = cell * (size_t)n_why;
#pragma unroll
    for (int s = 0; s < WHY_MAX; ++s) {
        const int i = s - (WHY_MAX - n_why);
        if (i < 0 || why_is_empty(l.k[s])) continue;
        d_src[base + i] = in_src[p0 + l.k[s].pos];
        d_term[base + i] = why_value(l.k[s].bits);
    }
}

// ---- the host side ----------------------------------------------------------------------------------------------------------------

int32_t why_prepare(rwr_graph *g, WhyEnd &w, int32_t K, int32_t top_n, hipStream_t s)
{
    const size_t cells = why_entry_cells(K, top_n), rcells = why_reason_cells(K, top_n, w.n_why);
    RWR_TRY(w.d_row.alloc(cells));
    RWR_HIP(hipMemsetAsync(w.d_row.p, 0xFF, cells * sizeof(int32_t), s));
    if (w.n_why > 0) {
        RWR_TRY(w.d_src.alloc(rcells));
        RWR_TRY(w.d_term.alloc(rcells));
        RWR_HIP(hipMemsetAsync(w.d_src.p, 0xFF, rcells * sizeof(int32_t), s));
        RWR_HIP(hipMemsetAsync(w.d_term.p, 0, rcells * sizeof(double), s));
    }
    if (w.why_total) {
        RWR_TRY(w.d_total.alloc(cells));
        RWR_HIP(hipMemsetAsync(w.d_total.p, 0, cells * sizeof(int64_t), s));
    }
    return RWR_OK;
}

int32_t why_rank_group(rwr_graph *g, WhyEnd &w, int G, int tg, const int32_t *slot_k, int32_t top_n, const double *X, hipStream_t s,
                       const int32_t *rows, int32_t nrows)
{
    SelState *st = nullptr;
    void *cand_v = nullptr;
    RWR_TRY(rank_group_levels(g, G, tg, top_n, X, slot_k, s, rows, nrows, sizeof(SelCandRow), &st, &cand_v));
    SelCandRow *cand = (SelCandRow *)cand_v;
    const unsigned nblk = cdiv((size_t)nrows, SEL_ROWS_PER_BLOCK);
    RWR_DISPATCH_G(G, hipLaunchKernelGGL(k_sel_collect_rows<GG>, dim3(nblk, tg), dim3(256), 0, s, g->n, nrows, rows, g->node_id.p, X, st,
                                         slot_k, cand));
    RWR_HIP(hipFuncSetAttribute((const void *)k_sel_sort_emit_rows, hipFuncAttributeMaxDynamicSharedMemorySize,
                                SEL_SLOTS * (int)sizeof(SelCandRow)));   // (per launch: the attribute is per device)
    hipLaunchKernelGGL(k_sel_sort_emit_rows, dim3(tg * G), dim3(256), SEL_SLOTS * sizeof(SelCandRow), s, slot_k, top_n, st, cand,
                       g->d_out_id.p, g->d_out_score.p, g->d_counts.p, w.d_row.p);
    RWR_HIP(hipGetLastError());
    return RWR_OK;
}

int32_t why_group(rwr_graph *g, WhyEnd &w, int G, int tg, const int32_t *slot_k, int32_t top_n, const double *Y, hipStream_t s)
{
    if (!w.reasons()) return RWR_OK;
    if (!Y) { set_error("rwr_recommend_explained_batch: the driver handed over no previous ranks"); return RWR_E_INVALID; }
    hipLaunchKernelGGL(k_why, dim3((unsigned)top_n, (unsigned)(tg * G)), dim3(WHY_BLOCK), 0, s, g->n, G, top_n, w.n_why, w.c1, slot_k,
                       g->d_counts.p, w.d_row.p, Y, g->in_ptr.p, g->in_src.p, g->vf ? (const double *)nullptr : g->in_w.p, g->w_src.p,
                       w.d_src.p, w.d_term.p, w.why_total ? w.d_total.p : (int64_t *)nullptr);
    RWR_HIP(hipGetLastError());
    return RWR_OK;
}

int32_t why_copy_back(rwr_graph *g, WhyEnd &w, int32_t K, int32_t top_n)
{
    hipStream_t s = g->stream;
    const size_t cells = why_entry_cells(K, top_n), rcells = why_reason_cells(K, top_n, w.n_why);
    if (w.nodes) RWR_HIP(hipMemcpyAsync(w.nodes, w.d_row.p, cells * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (w.n_why > 0) {
        RWR_HIP(hipMemcpyAsync(w.why_src, w.d_src.p, rcells * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        RWR_HIP(hipMemcpyAsync(w.why_term, w.d_term.p, rcells * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    if (w.why_total) RWR_HIP(hipMemcpyAsync(w.why_total, w.d_total.p, cells * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    RWR_HIP(hipStreamSynchronize(s));
    return RWR_OK;
}

}  // namespace rwr
