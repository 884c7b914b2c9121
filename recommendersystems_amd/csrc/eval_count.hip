// Hits / average precision of a tile group's walks without a ranked list (rwr_recommend_restart_eval_batch).
//
// Experiment.cs:121-128 walks a ranked list and adds (double)nHits / (i + 1) at every hit.  The position i of a hit is the
// number of candidates that rank before it, and the candidates between two hits need no order among themselves: so the group
// is evaluated by
//   1. hits     every candidate (row of the candidate list whose element of X is not the exclusion marker) looks its node id up in its slot's
//               sorted test set; a hit appends its 128-bit (score, id) key to the slot's list, sized exactly by a counting launch;
//   2. sort     the slots' hit keys descending: sel_sort in one workgroup up to SEL_SLOTS keys, sort.hip's radix sort above;
//   3. count    every candidate finds by binary search how many hit keys are >= its own and adds one to that interval's
//               counter (LDS-private per workgroup while the tile's lists fit, global otherwise);
//   4. finish   one workgroup per slot: a prefix sum over the intervals gives every hit its position; one thread adds the
//               addends in rank order (eval_ranked_body's division and summation order).  The positions destination
//               (eval_pos.hip) runs stages 1-3 as they are (eval_count_group) and a finish of its own.
// Integer counting only: the result does not depend on scheduling.  Stages 1 and 3 read the group's candidate rows of X once
// each; nothing of size K x candidates is written.  The candidate list is the caller's: the ITEM rows for the restart batch,
// the cached rows of a node type for rwr_recommend_typed_eval_batch.
#include "eval_count.h"
#include "rank_keys.h"

namespace rwr {

static_assert(EVAL_SORT_SLOTS == SEL_SLOTS, "the one-workgroup sort holds SEL_SLOTS keys");

__device__ __forceinline__ bool key_ge(const SelCand &a, const SelCand &b)
{
    return a.hi > b.hi || (a.hi == b.hi && a.lo >= b.lo);
}

// Stage 1.  Thread = (lane k of the tile, row lane rl): the G slots of a row read consecutive elements of X.  FILL = false
// counts the hits of every slot into cnt; FILL = true appends their keys at hits[hit_off[slot] + cursor[slot]++].
template <int G, bool FILL>
__global__ __launch_bounds__(256) void k_eval_hits(int32_t n, int32_t nrows, const int32_t *__restrict__ rows,
                                                   const int64_t *__restrict__ node_id, const double *__restrict__ X,
                                                   const int32_t *__restrict__ slot_k, const int64_t *__restrict__ ids,
                                                   const int64_t *__restrict__ slot_off, int32_t *__restrict__ cnt,
                                                   const int64_t *__restrict__ hit_off, int32_t *__restrict__ cursor,
                                                   SelCand *__restrict__ hits, int32_t *__restrict__ flag)
{
    constexpr int RL = 256 / G;
    const int tile = blockIdx.y;
    const int tid = threadIdx.x, k = tid % G, rl = tid / G;
    const int slot = tile * G + k;
    if (slot_k[slot] < 0) return;
    const int64_t t0 = slot_off[slot];
    const int32_t nt = (int32_t)(slot_off[slot + 1] - t0);
    if (nt == 0) return;
    const int64_t *ts = ids + t0;
    const double *x = X + (size_t)tile * (size_t)n * G;
    const int32_t q0 = blockIdx.x * SEL_ROWS_PER_BLOCK;
    const int32_t q1 = (q0 + SEL_ROWS_PER_BLOCK < nrows) ? q0 + SEL_ROWS_PER_BLOCK : nrows;
    int32_t mine = 0;
    for (int32_t q = q0 + rl; q < q1; q += RL) {
        const int32_t row = rows[q];
        const double s = x[(size_t)row * G + k];
        if (!(s >= 0.0)) continue;                                   // excluded (Recommender.cs:29)
        const int64_t id = node_id[row];
        int32_t lo = 0, hi = nt;                                     // testSet.Contains (Experiment.cs:124)
        while (lo < hi) {
            const int32_t mid = lo + (hi - lo) / 2;
            if (ts[mid] < id) lo = mid + 1;
            else hi = mid;
        }
        if (lo == nt || ts[lo] != id) continue;
        if (!FILL) { ++mine; continue; }
        const int64_t h0 = hit_off[slot];
        const int32_t cap = (int32_t)(hit_off[slot + 1] - h0);
        const int32_t pos = atomicAdd(&cursor[slot], 1);
        if (pos < cap) hits[h0 + pos] = SelCand{f64_orderable(s), i64_orderable(id)};
        else *flag = 1;
    }
    if (!FILL && mine) atomicAdd(&cnt[slot], mine);
}

// Stage 2, lists of up to SEL_SLOTS keys: one workgroup per slot
__global__ __launch_bounds__(256) void k_eval_sort_small(const int64_t *__restrict__ hit_off, const SelCand *__restrict__ hits,
                                                         SelCand *__restrict__ sorted)
{
    extern __shared__ SelCand sc[];
    const int64_t h0 = hit_off[blockIdx.x];
    const int64_t c64 = hit_off[blockIdx.x + 1] - h0;
    if (c64 == 0 || c64 > SEL_SLOTS) return;
    const int cnt = (int)c64;
    int N2 = 1;
    while (N2 < cnt) N2 <<= 1;
    for (int i = threadIdx.x; i < N2; i += blockDim.x) sc[i] = (i < cnt) ? hits[h0 + i] : SelCand{0ull, 0ull};
    __syncthreads();
    sel_sort(sc, N2);
    for (int i = threadIdx.x; i < cnt; i += blockDim.x) sorted[h0 + i] = sc[i];
}

// ... longer lists: the 128-bit key through two stable 64-bit radix sorts (id, then score), ascending, then turned round.
// half = 0: keys[i] = id key of hits[i], vals[i] = i;  half = 1: keys[i] = score key of hits[perm[i]], vals[i] = perm[i]
__global__ __launch_bounds__(256) void k_eval_radix_keys(const SelCand *__restrict__ hits, int32_t cnt, int half,
                                                         const uint32_t *__restrict__ perm, uint64_t *__restrict__ keys,
                                                         uint32_t *__restrict__ vals)
{
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cnt) return;
    const uint32_t src = half ? perm[i] : (uint32_t)i;
    keys[i] = half ? hits[src].hi : hits[src].lo;
    vals[i] = src;
}
__global__ __launch_bounds__(256) void k_eval_radix_gather(const SelCand *__restrict__ hits, int32_t cnt,
                                                           const uint32_t *__restrict__ perm, SelCand *__restrict__ sorted)
{
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < cnt) sorted[i] = hits[perm[cnt - 1 - i]];
}

// Stage 3.  A candidate with key c belongs to interval j = number of the slot's hit keys >= c (a prefix of the descending
// list): the candidates that rank strictly before hit i are those of the intervals 0 .. f, f being the first hit with hit i's
// key.  A thread keeps the run of its last interval in a register: most candidates of a slot fall below its last hit.
template <int G>
__global__ __launch_bounds__(256) void k_eval_count(int32_t n, int32_t nrows, const int32_t *__restrict__ rows,
                                                    const int64_t *__restrict__ node_id, const double *__restrict__ X,
                                                    const int32_t *__restrict__ slot_k, const int64_t *__restrict__ hit_off,
                                                    const SelCand *__restrict__ sorted, const uint8_t *__restrict__ tile_lds,
                                                    uint32_t *__restrict__ counters)
{
    constexpr int RL = 256 / G;
    extern __shared__ SelCand lds_keys[];
    const int tile = blockIdx.y;
    const int tid = threadIdx.x, k = tid % G, rl = tid / G;
    const int s0 = tile * G, slot = s0 + k;
    const int64_t h0 = hit_off[s0];
    const int64_t hT = hit_off[s0 + G] - h0;
    const bool in_lds = tile_lds[tile] != 0;                        // (then hT * 20 + G * 4 bytes fit: eval_group_layout)
    uint32_t *lds_cnt = (uint32_t *)(lds_keys + (in_lds ? hT : 0));
    if (in_lds) {
        for (int64_t i = tid; i < hT; i += 256) lds_keys[i] = sorted[h0 + i];
        for (int64_t i = tid; i < hT + G; i += 256) lds_cnt[i] = 0;
        __syncthreads();
    }
    uint32_t *gcnt = counters + h0 + s0;                             // the tile's hT + G counters
    if (slot_k[slot] >= 0) {
        const int64_t my0 = hit_off[slot] - h0;
        const int32_t my_h = (int32_t)(hit_off[slot + 1] - hit_off[slot]);
        const SelCand *keys = in_lds ? lds_keys + my0 : sorted + h0 + my0;
        uint32_t *cn = (in_lds ? lds_cnt : gcnt) + my0 + k;          // my_h + 1 counters
        const double *x = X + (size_t)tile * (size_t)n * G;
        const int32_t q0 = blockIdx.x * SEL_ROWS_PER_BLOCK;
        const int32_t q1 = (q0 + SEL_ROWS_PER_BLOCK < nrows) ? q0 + SEL_ROWS_PER_BLOCK : nrows;
        int32_t run_j = 0;
        uint32_t run_n = 0;
        for (int32_t q = q0 + rl; q < q1; q += RL) {
            const int32_t row = rows[q];
            const double s = x[(size_t)row * G + k];
            if (!(s >= 0.0)) continue;
            int32_t lo = 0, hi = my_h;
            if (my_h > 0) {
                const SelCand c{f64_orderable(s), i64_orderable(node_id[row])};
                while (lo < hi) {
                    const int32_t mid = lo + (hi - lo) / 2;
                    if (key_ge(keys[mid], c)) lo = mid + 1;
                    else hi = mid;
                }
            }
            if (lo == run_j) { ++run_n; continue; }
            if (run_n) atomicAdd(&cn[run_j], run_n);
            run_j = lo;
            run_n = 1;
        }
        if (run_n) atomicAdd(&cn[run_j], run_n);
    }
    if (in_lds) {
        __syncthreads();
        for (int64_t i = tid; i < hT + G; i += 256) {
            const uint32_t v = lds_cnt[i];
            if (v) atomicAdd(&gcnt[i], v);
        }
    }
}

// Stage 4: one workgroup per slot.  The counters become their inclusive prefix sums in place; hit i (first of its key: f) lies
// at position prefix[f] + (i - f); hits at or beyond top_n (> 0) drop out -- positions grow with i, so they are a tail.
__global__ __launch_bounds__(256) void k_eval_finish(const int32_t *__restrict__ slot_k, const int64_t *__restrict__ hit_off,
                                                     const SelCand *__restrict__ sorted, uint32_t *__restrict__ counters,
                                                     double *__restrict__ terms, int32_t top_n, EvalOut *__restrict__ out)
{
    __shared__ uint32_t sh[256];
    __shared__ uint32_t carry;
    __shared__ int kept;
    const int slot = blockIdx.x, tid = threadIdx.x;
    const int32_t orow = slot_k[slot];                              // batch position of this slot's vector
    if (orow < 0) return;
    const int64_t h0 = hit_off[slot];
    const int32_t h = (int32_t)(hit_off[slot + 1] - h0);
    uint32_t *c = counters + h0 + slot;
    const SelCand *keys = sorted + h0;
    double *tm = terms + h0;
    if (tid == 0) kept = 0;
    eval_prefix_counters(c, h, sh, &carry);
    int mine = 0;
    for (int32_t i = tid; i < h; i += 256) {
        int32_t f = i;
        while (f > 0 && keys[f - 1].hi == keys[i].hi && keys[f - 1].lo == keys[i].lo) --f;
        const int64_t pos = (int64_t)c[f] + (i - f);
        if (top_n > 0 && pos >= top_n) continue;
        tm[i] = (double)(i + 1) / (double)(pos + 1);                // (double)nHits / (i + 1)  (Experiment.cs:126)
        ++mine;
    }
    if (mine) atomicAdd(&kept, mine);
    __syncthreads();
    if (tid == 0) {
        const int nh = kept;
        double sum = 0.0;
        for (int i = 0; i < nh; ++i) sum += tm[i];                  // sumPrecision += ... in rank order
        const int64_t len = carry;
        out[orow] = EvalOut{nh, sum, (top_n > 0 && len > top_n) ? (int64_t)top_n : len};
    }
}

int32_t eval_plan_upload(EvalEnd &ev, int32_t K, const std::vector<int32_t> &slot_k, size_t slots_per_group, const void *out_a,
                         const void *out_b, const char *who, hipStream_t s)
{
    ev.plan = eval_plan(slot_k.size(), slot_k.data(), slots_per_group, K, ev.test_ptr, ev.test_ids, out_a, out_b);
    if (ev.plan.check.verdict != EVAL_OK) {                        // (api.hip refuses such sets before the call gets here)
        set_error("%s: test sets failed their check (verdict %d)", who, (int)ev.plan.check.verdict);
        return RWR_E_INVALID;
    }
    RWR_TRY(ev.d_ids.alloc(ev.plan.n_ids));
    RWR_TRY(ev.d_slot_off.alloc(ev.plan.n_off));
    RWR_TRY(ev.d_flag.alloc(1));
    RWR_TRY(ev.d_cnt.alloc(ev.plan.n_group_slots));
    RWR_TRY(ev.d_cursor.alloc(ev.plan.n_group_slots));
    RWR_TRY(ev.d_hit_off.alloc(ev.plan.n_group_slots + 1));
    RWR_TRY(ev.d_tile_lds.alloc(ev.plan.n_group_slots));
    if (ev.plan.n_ids > 0)
        RWR_HIP(hipMemcpyAsync(ev.d_ids.p, ev.plan.ids.data(), ev.plan.n_ids * sizeof(int64_t), hipMemcpyHostToDevice, s));
    RWR_HIP(hipMemcpyAsync(ev.d_slot_off.p, ev.plan.slot_off.data(), ev.plan.n_off * sizeof(int64_t), hipMemcpyHostToDevice, s));
    RWR_HIP(hipMemsetAsync(ev.d_flag.p, 0, sizeof(int32_t), s));
    return RWR_OK;
}

int32_t eval_prepare(rwr_graph *g, EvalEnd &ev, int32_t K, const std::vector<int32_t> &slot_k, size_t slots_per_group,
                     const char *who, hipStream_t s)
{
    RWR_TRY(eval_plan_upload(ev, K, slot_k, slots_per_group, ev.n_hits, ev.sum_precision, who, s));
    RWR_TRY(ev.d_out.alloc(ev.plan.n_out));
    RWR_HIP(hipMemsetAsync(ev.d_out.p, 0, ev.plan.n_out * sizeof(EvalOut), s));
    return RWR_OK;
}

// the radix sort of one long hit list (cnt keys at hits, descending into sorted), in the handle's sort buffers
static int32_t sort_long(rwr_graph *g, const SelCand *hits, int32_t cnt, SelCand *sorted, hipStream_t s)
{
    const size_t m = (size_t)cnt;
    RWR_TRY(g->keys.ensure(m));
    RWR_TRY(g->keys_alt.ensure(m));
    RWR_TRY(g->vals.ensure(m));
    RWR_TRY(g->vals_alt.ensure(m));
    RWR_TRY(g->sort_temp.ensure(radix_sort_temp_bytes(m, 1)));
    const dim3 grid(cdiv(m, 256));
    hipLaunchKernelGGL(k_eval_radix_keys, grid, dim3(256), 0, s, hits, cnt, 0, (const uint32_t *)nullptr, g->keys.p, g->vals.p);
    bool alt = false;
    RWR_TRY(radix_sort_pairs<uint64_t>(g->keys.p, g->keys_alt.p, g->vals.p, g->vals_alt.p, m, 1, 64, g->sort_temp.p, s, &alt));
    // the id order is the payload of the side the sort ended on; the score keys go to the other side, which is sorted next
    uint64_t *ka = alt ? g->keys.p : g->keys_alt.p, *kb = alt ? g->keys_alt.p : g->keys.p;
    uint32_t *va = alt ? g->vals.p : g->vals_alt.p, *vb = alt ? g->vals_alt.p : g->vals.p;
    hipLaunchKernelGGL(k_eval_radix_keys, grid, dim3(256), 0, s, hits, cnt, 1, (const uint32_t *)vb, ka, va);
    RWR_TRY(radix_sort_pairs<uint64_t>(ka, kb, va, vb, m, 1, 64, g->sort_temp.p, s, &alt));
    hipLaunchKernelGGL(k_eval_radix_gather, grid, dim3(256), 0, s, hits, cnt, (const uint32_t *)(alt ? vb : va), sorted);
    RWR_HIP(hipGetLastError());
    return RWR_OK;
}

int32_t eval_count_group(rwr_graph *g, EvalEnd &ev, int G, int tg, size_t q0, const double *X, const int32_t *rows, int32_t nrows,
                         hipStream_t s)
{
    const int32_t m = nrows;
    const size_t S = (size_t)tg * G;
    const int32_t *slot_k = g->d_slot_k.p + q0;
    const int64_t *slot_off = ev.d_slot_off.p + q0;
    const dim3 grid(cdiv((size_t)m, SEL_ROWS_PER_BLOCK), (unsigned)tg);
    // 1. the slots' hit counts, then the exact layout of the group's lists and counters
    RWR_HIP(hipMemsetAsync(ev.d_cnt.p, 0, S * sizeof(int32_t), s));
    RWR_DISPATCH_G(G, hipLaunchKernelGGL((k_eval_hits<GG, false>), grid, dim3(256), 0, s, g->n, m, rows, g->node_id.p, X,
                                         slot_k, ev.d_ids.p, slot_off, ev.d_cnt.p, (const int64_t *)nullptr,
                                         (int32_t *)nullptr, (SelCand *)nullptr, (int32_t *)nullptr));
    RWR_HIP(hipGetLastError());
    ev.h_cnt.assign(S, 0);
    RWR_HIP(hipMemcpyAsync(ev.h_cnt.data(), ev.d_cnt.p, S * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    RWR_HIP(hipStreamSynchronize(s));                               // (the earlier groups' kernels are through as well)
    ev.layout = eval_group_layout(ev.h_cnt.data(), S, G);
    const EvalGroupLayout &L = ev.layout;
    if (L.bad || L.n_counters > 0xFFFFFFFFll) { set_error("evaluation: a tile group's hit lists are out of range"); return RWR_E_UNSUPPORTED; }
    RWR_TRY(ev.d_hits.ensure((size_t)L.n_hits * sizeof(SelCand)));
    RWR_TRY(ev.d_sorted.ensure((size_t)L.n_hits * sizeof(SelCand)));
    RWR_TRY(ev.d_counters.ensure((size_t)L.n_counters));
    SelCand *hits = (SelCand *)ev.d_hits.p, *sorted = (SelCand *)ev.d_sorted.p;
    RWR_HIP(hipMemcpyAsync(ev.d_hit_off.p, L.hit_off.data(), (S + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
    RWR_HIP(hipMemcpyAsync(ev.d_tile_lds.p, L.tile_lds.data(), (size_t)tg, hipMemcpyHostToDevice, s));
    if (L.n_hits > 0) {
        RWR_HIP(hipMemsetAsync(ev.d_cursor.p, 0, S * sizeof(int32_t), s));
        RWR_DISPATCH_G(G, hipLaunchKernelGGL((k_eval_hits<GG, true>), grid, dim3(256), 0, s, g->n, m, rows, g->node_id.p,
                                             X, slot_k, ev.d_ids.p, slot_off, (int32_t *)nullptr, ev.d_hit_off.p,
                                             ev.d_cursor.p, hits, ev.d_flag.p));
        // 2. sorted descending
        int32_t longest_short = 0;
        for (size_t q = 0; q < S; ++q)
            if (ev.h_cnt[q] <= SEL_SLOTS && ev.h_cnt[q] > longest_short) longest_short = ev.h_cnt[q];
        if (longest_short > 0) {
            int N2 = 1;
            while (N2 < longest_short) N2 <<= 1;
            (void)hipFuncSetAttribute((const void *)k_eval_sort_small, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      SEL_SLOTS * (int)sizeof(SelCand));
            hipLaunchKernelGGL(k_eval_sort_small, dim3((unsigned)S), dim3(256), (size_t)N2 * sizeof(SelCand), s, ev.d_hit_off.p,
                               hits, sorted);
        }
        RWR_HIP(hipGetLastError());
        for (const int32_t q : L.long_slots)
            RWR_TRY(sort_long(g, hits + L.hit_off[(size_t)q], ev.h_cnt[(size_t)q], sorted + L.hit_off[(size_t)q], s));
    }
    // 3. the interval counters; a tile whose lists fit keeps them in LDS
    RWR_HIP(hipMemsetAsync(ev.d_counters.p, 0, (size_t)L.n_counters * sizeof(uint32_t), s));
    size_t lds = 0;
    for (int t = 0; t < tg; ++t)
        if (L.tile_lds[(size_t)t]) {
            const size_t hT = (size_t)(L.hit_off[(size_t)(t + 1) * G] - L.hit_off[(size_t)t * G]);
            lds = std::max(lds, hT * sizeof(SelCand) + (hT + (size_t)G) * sizeof(uint32_t));
        }
    RWR_DISPATCH_G(G, {
        (void)hipFuncSetAttribute((const void *)k_eval_count<GG>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)EVAL_LDS_BYTES);
        hipLaunchKernelGGL(k_eval_count<GG>, grid, dim3(256), lds, s, g->n, m, rows, g->node_id.p, X, slot_k,
                           ev.d_hit_off.p, sorted, ev.d_tile_lds.p, ev.d_counters.p);
    });
    RWR_HIP(hipGetLastError());
    return RWR_OK;
}

int32_t eval_group(rwr_graph *g, EvalEnd &ev, int G, int tg, size_t q0, const double *X, const int32_t *rows, int32_t nrows,
                   hipStream_t s)
{
    if (nrows == 0) return RWR_OK;                                  // no candidate anywhere: the zeroed records stand
    RWR_TRY(eval_count_group(g, ev, G, tg, q0, X, rows, nrows, s));
    // 4. positions, addends in rank order, the records at the vectors' batch positions
    RWR_TRY(ev.d_terms.ensure((size_t)ev.layout.n_hits));
    hipLaunchKernelGGL(k_eval_finish, dim3((unsigned)tg * G), dim3(256), 0, s, g->d_slot_k.p + q0, ev.d_hit_off.p,
                       (const SelCand *)ev.d_sorted.p, ev.d_counters.p, ev.d_terms.p, ev.top_n, ev.d_out.p);
    RWR_HIP(hipGetLastError());
    return RWR_OK;
}

int32_t eval_copy_back(rwr_graph *g, EvalEnd &ev, int32_t K, const char *who, hipStream_t s)
{
    std::vector<EvalOut> out((size_t)K);
    int32_t flag = 0;
    RWR_HIP(hipMemcpyAsync(out.data(), ev.d_out.p, (size_t)K * sizeof(EvalOut), hipMemcpyDeviceToHost, s));
    RWR_HIP(hipMemcpyAsync(&flag, ev.d_flag.p, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    RWR_HIP(hipStreamSynchronize(s));
    if (flag) { set_error("%s: a hit list overflowed its counted size", who); return RWR_E_HIP; }
    for (int32_t k = 0; k < K; ++k) {
        ev.n_hits[k] = out[(size_t)k].n_hits;
        ev.sum_precision[k] = out[(size_t)k].sum_precision;
        if (ev.list_len) ev.list_len[k] = out[(size_t)k].list_len;
    }
    return RWR_OK;
}

}  // namespace rwr
