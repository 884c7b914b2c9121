// Positions and scores of the test ids of a tile group's walks (rwr_recommend_typed_positions_batch,
// rwr_recommend_restart_typed_positions_batch).
//
// The counting evaluation (eval_count.hip) knows the position of every hit after its third stage and folds them into one
// number in its fourth.  This destination keeps them instead: stages 1-3 run as they are (eval_count_group), and in place
// of k_eval_finish one workgroup per slot
//   - turns the slot's interval counters into their prefix sums (eval_prefix_counters, the finish they share);
//   - gives hit i, whose first equal key is f, the position c[f] + (i - f), takes its id and score back out of the key and
//     finds the id's place u in the slot's sorted set by bisection (the lookup that made it a hit);
//   - of the hits that carry one id (node ids need not be unique) lets the best-ranked one answer: an integer minimum over the
//     positions, then, behind a barrier, the hit whose position won writes its score.  Positions of distinct hits differ, so
//     exactly one hit writes; nothing depends on the order in which the workgroup's waves run.
// The result arrays are parallel to the plan's laid-out ids and start at -1 / +0.0: an id that nothing carries, or whose
// candidates are all excluded, keeps them.  pos_plan.h maps the caller's entries (their order, their duplicates) onto them.
#include "eval_pos.h"
#include "rank_keys.h"

namespace rwr {

// -1 as an unsigned word is the largest one: the initial "no hit" loses every minimum
static_assert((unsigned long long)(int64_t)-1 == ~0ull, "the positions' initial value must lose an unsigned minimum");

__device__ __forceinline__ int64_t pos_of_hit(const SelCand *keys, const uint32_t *c, int32_t i)
{
    int32_t f = i;
    while (f > 0 && keys[f - 1].hi == keys[i].hi && keys[f - 1].lo == keys[i].lo) --f;
    return (int64_t)c[f] + (i - f);
}

// the place of id in the ascending set ts[0 .. nt), -1 if it is not there
__device__ __forceinline__ int32_t pos_place(const int64_t *ts, int32_t nt, int64_t id)
{
    int32_t lo = 0, hi = nt;
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo) / 2;
        if (ts[mid] < id) lo = mid + 1;
        else hi = mid;
    }
    return (lo < nt && ts[lo] == id) ? lo : -1;
}

__global__ __launch_bounds__(256) void k_pos_finish(const int32_t *__restrict__ slot_k, const int64_t *__restrict__ hit_off,
                                                    const SelCand *__restrict__ sorted, uint32_t *__restrict__ counters,
                                                    const int64_t *__restrict__ ids, const int64_t *__restrict__ slot_off,
                                                    int64_t *pos, double *__restrict__ score, int64_t *__restrict__ len)
{
    __shared__ uint32_t sh[256];
    __shared__ uint32_t carry;
    const int slot = blockIdx.x, tid = threadIdx.x;
    const int32_t orow = slot_k[slot];                              // batch position of this slot's vector
    if (orow < 0) return;
    const int64_t h0 = hit_off[slot];
    const int32_t h = (int32_t)(hit_off[slot + 1] - h0);
    uint32_t *c = counters + h0 + slot;
    const SelCand *keys = sorted + h0;
    const int64_t t0 = slot_off[slot];
    const int32_t nt = (int32_t)(slot_off[slot + 1] - t0);
    const int64_t *ts = ids + t0;
    unsigned long long *best = (unsigned long long *)(pos + t0);
    eval_prefix_counters(c, h, sh, &carry);
    for (int32_t i = tid; i < h; i += 256) {
        int64_t id;
        double sc;
        sel_decode(keys[i], &id, &sc);
        const int32_t u = pos_place(ts, nt, id);
        if (u >= 0) atomicMin(&best[u], (unsigned long long)pos_of_hit(keys, c, i));
    }
    __threadfence();                                                // the minima are in memory before anyone reads them back
    __syncthreads();
    for (int32_t i = tid; i < h; i += 256) {
        int64_t id;
        double sc;
        sel_decode(keys[i], &id, &sc);
        const int32_t u = pos_place(ts, nt, id);
        if (u < 0) continue;
        const unsigned long long won = __hip_atomic_load(&best[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (won == (unsigned long long)pos_of_hit(keys, c, i)) score[t0 + u] = sc;
    }
    if (tid == 0) len[orow] = (int64_t)carry;
}

int32_t pos_prepare(rwr_graph *g, PosEnd &pe, int32_t K, const std::vector<int32_t> &slot_k, size_t slots_per_group,
                    const char *who, hipStream_t s)
{
    EvalEnd &ev = pe.ev;
    RWR_TRY(eval_plan_upload(ev, K, slot_k, slots_per_group, pe.pos_out, pe.pos_out, who, s));
    pe.plan = pos_plan(ev.plan, slot_k.size(), slot_k.data(), K, ev.test_ptr, ev.test_ids);
    RWR_TRY(pe.d_pos.alloc(pe.plan.n_pos));
    RWR_TRY(pe.d_score.alloc(pe.plan.n_score));
    RWR_TRY(pe.d_len.alloc(pe.plan.n_len));
    if (pe.plan.n_pos > 0) {
        RWR_HIP(hipMemsetAsync(pe.d_pos.p, 0xFF, pe.plan.n_pos * sizeof(int64_t), s));      // -1: no candidate carries the id
        RWR_HIP(hipMemsetAsync(pe.d_score.p, 0, pe.plan.n_score * sizeof(double), s));      // +0.0
    }
    RWR_HIP(hipMemsetAsync(pe.d_len.p, 0, pe.plan.n_len * sizeof(int64_t), s));
    return RWR_OK;
}

int32_t pos_group(rwr_graph *g, PosEnd &pe, int G, int tg, size_t q0, const double *X, const int32_t *rows, int32_t nrows,
                  hipStream_t s)
{
    if (nrows == 0) return RWR_OK;                                  // no candidate anywhere: -1 / +0.0 and the lengths 0 stand
    EvalEnd &ev = pe.ev;
    RWR_TRY(eval_count_group(g, ev, G, tg, q0, X, rows, nrows, s));
    hipLaunchKernelGGL(k_pos_finish, dim3((unsigned)tg * G), dim3(256), 0, s, g->d_slot_k.p + q0, ev.d_hit_off.p,
                       (const SelCand *)ev.d_sorted.p, ev.d_counters.p, ev.d_ids.p, ev.d_slot_off.p + q0, pe.d_pos.p, pe.d_score.p,
                       pe.d_len.p);
    RWR_HIP(hipGetLastError());
    return RWR_OK;
}

int32_t pos_copy_back(rwr_graph *g, PosEnd &pe, int32_t K, const char *who, hipStream_t s)
{
    std::vector<int64_t> pos(pe.plan.n_pos), len(pe.plan.n_len);
    std::vector<double> score(pe.plan.n_score);
    int32_t flag = 0;
    if (pe.plan.n_pos > 0) {
        RWR_HIP(hipMemcpyAsync(pos.data(), pe.d_pos.p, pos.size() * sizeof(int64_t), hipMemcpyDeviceToHost, s));
        RWR_HIP(hipMemcpyAsync(score.data(), pe.d_score.p, score.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    RWR_HIP(hipMemcpyAsync(len.data(), pe.d_len.p, len.size() * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    RWR_HIP(hipMemcpyAsync(&flag, pe.ev.d_flag.p, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    RWR_HIP(hipStreamSynchronize(s));
    if (flag) { set_error("%s: a hit list overflowed its counted size", who); return RWR_E_HIP; }
    pos_scatter(pe.plan, K, pos.data(), score.data(), len.data(), pe.pos_out, pe.score_out, pe.list_len);
    return RWR_OK;
}

}  // namespace rwr
