// Model with a caller-set restart vector (the public field Model.restart, Model.cs:12; read by deliverRanks at Model.cs:92-93
// for rows with links and :96-97 for dangling rows).  include/rwr.h: rwr_model_run_restart / rwr_model_deliver_restart.
//
// One deliverRanks with restart vector v leaves, for every row r,
//     next[r] = fold over i = 0..n-1 of ( links of i into r in list order: fl(fl((1-d) x_i) * w) ; then fl(rr_i * v[r]) )
// with rr_i = x_i - fl((1-d) x_i) for a row with links, rr_i = x_i for a dangling row, starting at +0.0.  A row outside the
// support S = {r : v[r] != 0} only receives restart addends rr_i * 0 = +-0, which leave a fold that starts at +0.0 unchanged
// while every rr_i is finite: those rows are the link-only fold the single-seed SpMV computes (seed -1).  Each row of S is an
// n-term chain of its own:
//   |S| <= RWR_RESTART_EXACT_MAX   k_restart_fold, one wave per support row beside the link-only SpMV, bitwise;
//   |S| >  RWR_RESTART_EXACT_MAX   link-only SpMV + (tree-summed restart mass) * v[r], tolerance parity like the global model.
#include <algorithm>
#include <cmath>

#include "iterate.h"

namespace rwr {

// One round of k_restart_fold folds the next RS_W addends of the row's merged sequence: the restart addends of rows
// i, i+1, ... and the in-links of the row (sorted by source) from p on, merged by (source row, link before restart).
constexpr int RS_E = 8;                 // rows and links per lane and round
constexpr int RS_W = WAVE * RS_E;       // addends per round

struct FoldWindow {
    double xr[RS_E];       // x of rows i + lane*RS_E + e
    uint8_t dg[RS_E];      // ... dangling flags
    int32_t src[RS_E];     // source of link p + lane*RS_E + e (INT32_MAX past the row's last link)
    double w[RS_E];
};

// (indices clamped instead of branches: the loads issue back to back and are waited for only where they are used; a
// position past the end reads element 0 -- every buffer holds at least one -- and is masked)
// (xs: distance between consecutive rows of X in doubles -- 1 for a rank vector, G for a column of a tile)
__device__ __forceinline__ void fold_load(FoldWindow &f, int64_t i, int64_t p, int32_t n, int64_t pe, int lane,
                                          const double *__restrict__ X, size_t xs, const uint8_t *__restrict__ dangling,
                                          const int32_t *__restrict__ in_src, const double *__restrict__ in_w)
{
#pragma unroll
    for (int e = 0; e < RS_E; ++e) {
        const int64_t q = i + lane * RS_E + e;
        const int64_t qc = q < n ? q : 0;
        f.xr[e] = X[(size_t)qc * xs];
        f.dg[e] = dangling[qc];
        const int64_t l = p + lane * RS_E + e;
        const int64_t lc = l < pe ? l : 0;
        const int32_t sv = in_src[lc];
        f.src[e] = l < pe ? sv : INT32_MAX;
        f.w[e] = in_w[lc];
    }
}

__device__ __forceinline__ int wave_sum(int v)
{
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) v += __shfl_xor(v, o);
    return v;
}

// next[r] of one support row r with restart value v, by one wave (bitwise the reference's fold).  Every addend is formed in
// parallel (64 lanes x RS_E rows, the same for links), placed at its position in the merged sequence through LDS, and lane
// 0 adds the round's RS_W addends strictly in order.  The next round's rows and links are loaded before that serial fold,
// so their latency hides behind it.  Merge-path: the first RS_W addends of the merged remainder lie inside the two
// RS_W-wide windows, and their window-local positions are their true positions.  X: rank of row q at X[q * xs].
// The result is valid in lane 0.
__device__ __forceinline__ double restart_fold_row(int32_t n, int32_t r, double v, const int64_t *__restrict__ in_ptr,
                                                   const int32_t *__restrict__ in_src, const double *__restrict__ in_w,
                                                   const double *__restrict__ X, size_t xs,
                                                   const uint8_t *__restrict__ dangling, double c1, double *seq, int32_t *cnt)
{
    const int lane = threadIdx.x;
    int64_t p = in_ptr[r];
    const int64_t pe = in_ptr[r + 1];
    int64_t i = 0;
    double acc = 0.0;
    FoldWindow f;
    fold_load(f, i, p, n, pe, lane, X, xs, dangling, in_src, in_w);
    while (i < n || p < pe) {
        const int64_t left = (pe - p) + ((int64_t)n - i);
        const int m = left < RS_W ? (int)left : RS_W;
#pragma unroll
        for (int e = 0; e < RS_E; ++e) cnt[lane * RS_E + e] = 0;
        __syncthreads();
        // links: position = own index + rows of the window in front of the source; count them per source row
        double lt[RS_E];
        int lpos[RS_E];
#pragma unroll
        for (int e = 0; e < RS_E; ++e) {
            const int64_t rel = (int64_t)f.src[e] - i;              // >= 0: links of rows before i are folded already
            const bool in = rel >= 0 && rel < RS_W;
            const double rw = c1 * X[(size_t)(in ? f.src[e] : r) * xs];   // Model.cs:84
            lt[e] = rw * f.w[e];                                    // Model.cs:87
            lpos[e] = in ? lane * RS_E + e + (int)rel : RS_W;
            if (in) atomicAdd(&cnt[rel], 1);
        }
        __syncthreads();
        // restart addends: position = own index + links of the window whose source is <= the row
        int c[RS_E], run = 0;
#pragma unroll
        for (int e = 0; e < RS_E; ++e) { run += cnt[lane * RS_E + e]; c[e] = run; }
        int incl = run;
#pragma unroll
        for (int o = 1; o < WAVE; o <<= 1) {
            const int t = __shfl_up(incl, o);
            if (lane >= o) incl += t;
        }
        const int before = incl - run;
        int took_rows = 0, took_links = 0;
#pragma unroll
        for (int e = 0; e < RS_E; ++e) {
            const int64_t q = i + lane * RS_E + e;
            const int pos = lane * RS_E + e + before + c[e];
            if (q < n && pos < m) {
                const double xq = f.xr[e];
                const double rr = f.dg[e] ? xq : (xq - c1 * xq);    // Model.cs:91 / :97
                seq[pos] = rr * v;                                  // Model.cs:93 / :97
                ++took_rows;
            }
            if (lpos[e] < m) {
                seq[lpos[e]] = lt[e];
                ++took_links;
            }
        }
        const int b = wave_sum(took_rows), a = wave_sum(took_links);
        __syncthreads();
        if (a + b != m) break;                                      // (cannot happen: the merge always advances)
        i += b;
        p += a;
        if (i < n || p < pe) fold_load(f, i, p, n, pe, lane, X, xs, dangling, in_src, in_w);
        if (lane == 0) {
#pragma unroll 8
            for (int t = 0; t < m; ++t) acc += seq[t];              // Model.cs:87 / :93 / :97, in order
        }
        __syncthreads();
    }
    return (i < n || p < pe) ? __builtin_nan("") : acc;
}

// grid = |S| one-wave workgroups; out[k] = next[sup[k]]
__global__ __launch_bounds__(WAVE) void k_restart_fold(int32_t n, const int32_t *__restrict__ sup, const double *__restrict__ vs,
                                                      const int64_t *__restrict__ in_ptr, const int32_t *__restrict__ in_src,
                                                      const double *__restrict__ in_w, const double *__restrict__ X,
                                                      const uint8_t *__restrict__ dangling, double c1, double *__restrict__ out)
{
    __shared__ double seq[RS_W];
    __shared__ int32_t cnt[RS_W];
    const double acc = restart_fold_row(n, sup[blockIdx.x], vs[blockIdx.x], in_ptr, in_src, in_w, X, 1, dangling, c1, seq, cnt);
    if (threadIdx.x == 0) out[blockIdx.x] = acc;
}

// The chains of a tile group of rwr_model_run_restart_batch (restart_batch.hip): one one-wave workgroup per
// (vector, support row) pair, every pair of the group in one launch.  Pair j: support row pr[j] with restart value pv[j] of
// the vector in slot pq[j] = tile * G + lane of the group's rank matrix X[tile][n][G] -- the same fold as k_restart_fold over
// column pq[j] of the interleaved tile (row q of the column at distance q * G).  The pairs are ordered by slot, so the
// chains that are resident together walk the same tile and share its 128-byte lines in the L2s.  6 KB of LDS, 116 VGPRs and
// one wave per workgroup: 16 chains are resident per CU.
__global__ __launch_bounds__(WAVE) void k_restart_fold_cols(int32_t n, int G, const int32_t *__restrict__ pq,
                                                           const int32_t *__restrict__ pr, const double *__restrict__ pv,
                                                           const int64_t *__restrict__ in_ptr, const int32_t *__restrict__ in_src,
                                                           const double *__restrict__ in_w, const double *__restrict__ X,
                                                           const uint8_t *__restrict__ dangling, double c1, double *__restrict__ out)
{
    __shared__ double seq[RS_W];
    __shared__ int32_t cnt[RS_W];
    const int32_t q = pq[blockIdx.x];
    const double *col = X + (size_t)(q / G) * (size_t)n * (size_t)G + (size_t)(q % G);
    const double acc = restart_fold_row(n, pr[blockIdx.x], pv[blockIdx.x], in_ptr, in_src, in_w, col, (size_t)G, dangling, c1, seq, cnt);
    if (threadIdx.x == 0) out[blockIdx.x] = acc;
}

// ... and replace the link-only values the SpMM wrote for them in Y[tile][n][G]
__global__ void k_restart_scatter_cols(int32_t npairs, int32_t n, int G, const int32_t *__restrict__ pq,
                                       const int32_t *__restrict__ pr, const double *__restrict__ fold, double *__restrict__ Y)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= npairs) return;
    const int32_t q = pq[j];
    Y[(size_t)(q / G) * (size_t)n * (size_t)G + (size_t)pr[j] * (size_t)G + (size_t)(q % G)] = fold[j];
}

// rank of a tile group's slots as the constructors leave it: st[slot] >= 0 personalised (Model.cs:44: n at the node, 0
// elsewhere), -1 global (Model.cs:25: every rank 1), -2 a padding slot (a zero column)
__global__ __launch_bounds__(256) void k_restart_init_cols(int32_t n, int G, int64_t elems, const int32_t *__restrict__ st,
                                                           double *__restrict__ X)
{
    const int64_t per_tile = (int64_t)n * G;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < elems; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t tile = i / per_tile, in_tile = i - tile * per_tile;
        const int32_t row = (int32_t)(in_tile / G), s = st[tile * G + in_tile % G];
        X[i] = s == -1 ? 1.0 : (s == row ? (double)n : 0.0);
    }
}

void launch_restart_fold_cols(rwr_graph *g, int G, int32_t npairs, const int32_t *pq, const int32_t *pr, const double *pv,
                              const double *X, double c1, double *fold, hipStream_t s)
{
    hipLaunchKernelGGL(k_restart_fold_cols, dim3((unsigned)npairs), dim3(WAVE), 0, s, g->n, G, pq, pr, pv, g->in_ptr.p, g->in_src.p,
                       g->in_w.p, X, g->dangling.p, c1, fold);
}
void launch_restart_scatter_cols(rwr_graph *g, int G, int32_t npairs, const int32_t *pq, const int32_t *pr, const double *fold,
                                 double *Y, hipStream_t s)
{
    hipLaunchKernelGGL(k_restart_scatter_cols, dim3(cdiv((size_t)npairs, 256)), dim3(256), 0, s, npairs, g->n, G, pq, pr, fold, Y);
}
void launch_restart_init_cols(rwr_graph *g, int G, int tg, const int32_t *st, double *X, hipStream_t s)
{
    const size_t elems = (size_t)tg * (size_t)g->n * (size_t)G;
    hipLaunchKernelGGL(k_restart_init_cols, dim3(std::min<size_t>(cdiv(elems, 256), 16384)), dim3(256), 0, s, g->n, G,
                       (int64_t)elems, st, X);
}

// the folded support rows replace the link-only values the SpMV wrote for them
__global__ void k_restart_scatter(int32_t nsup, const int32_t *__restrict__ sup, const double *__restrict__ fold,
                                  double *__restrict__ Y)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < nsup) Y[sup[k]] = fold[k];
}

// |S| > RWR_RESTART_EXACT_MAX: y[r] += M * v[r], M = tree-summed restart mass (the per-row form of k_add_restart_share)
__global__ void k_add_restart_vec(double *__restrict__ y, int32_t n, const double *__restrict__ total,
                                  const double *__restrict__ v)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] += *total * v[i];
}

static int32_t model_restart_body(rwr_graph *g, const double *v, const double *rank_in, double d, int32_t run_mode,
                                  double value, bool one_step, double *rank_out, int64_t *iters_out, const char *who)
{
    const int32_t n = g->n;
    for (int32_t i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) {
            set_error("%s: restart[%d] = %g is not finite (rr * 0 would be NaN in every row)", who, i, v[i]);
            return RWR_E_UNSUPPORTED;
        }
    bool ranks_nonneg = true, v_nonneg = true;
    for (int32_t i = 0; i < n; ++i) {
        if (!std::isfinite(rank_in[i])) {
            set_error("%s: rank[%d] = %g is not finite", who, i, rank_in[i]);
            return RWR_E_UNSUPPORTED;
        }
        ranks_nonneg = ranks_nonneg && rank_in[i] >= 0.0;
        v_nonneg = v_nonneg && v[i] >= 0.0;
    }
    std::vector<int32_t> sup;
    std::vector<double> vs;
    for (int32_t i = 0; i < n; ++i)
        if (v[i] != 0.0) { sup.push_back(i); vs.push_back(v[i]); }
    const int32_t nsup = (int32_t)sup.size();
    const bool exact = nsup <= RWR_RESTART_EXACT_MAX;
    const RunEnd end(run_mode, value, n);
    const double c1 = 1 - d;
    // every link addend >= 0 and finite (over a run the ranks stay >= 0 only when v >= 0 too): the SpMV may then sum hub rows
    // by the exact parallel reduction; otherwise its general kernels run (as rwr_model_deliver does for negative ranks)
    const bool hub_scan = c1 >= 0.0 && c1 <= 1.0 && g->nonneg && ranks_nonneg && (v_nonneg || one_step);
    hipStream_t s = g->stream, s2 = g->stream2;

    DevBuf<int32_t> d_sup;
    DevBuf<double> d_vs, d_fold, d_v;
    StreamsIdle idle{g};
    RWR_TRY(ensure_in_w(g));                                         // the link-only SpMV runs the weighted kernels
    RWR_TRY(g->X.ensure((size_t)n));
    RWR_TRY(g->Y.ensure((size_t)n));
    RWR_TRY(g->d_seeds.ensure(1));
    RWR_TRY(g->d_part.ensure(MODEL_RED_PARTS + 8));
    const int32_t no_seed = -1;
    RWR_HIP(hipMemcpyAsync(g->d_seeds.p, &no_seed, sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (exact && nsup > 0) {
        RWR_TRY(d_sup.alloc(nsup));
        RWR_TRY(d_vs.alloc(nsup));
        RWR_TRY(d_fold.alloc(nsup));
        RWR_HIP(hipMemcpyAsync(d_sup.p, sup.data(), sizeof(int32_t) * nsup, hipMemcpyHostToDevice, s));
        RWR_HIP(hipMemcpyAsync(d_vs.p, vs.data(), sizeof(double) * nsup, hipMemcpyHostToDevice, s));
    }
    if (!exact) {
        RWR_TRY(d_v.alloc((size_t)n));
        RWR_HIP(hipMemcpyAsync(d_v.p, v, sizeof(double) * n, hipMemcpyHostToDevice, s));
    }
    double *X = g->X.p, *Y = g->Y.p;
    SpmmArgs sp;                                                     // the link-only SpMV: no seed row, every row's links
    sp.seeds = g->d_seeds.p, sp.c1 = c1, sp.hub_scan = hub_scan;
    RWR_HIP(hipMemcpyAsync(X, rank_in, sizeof(double) * n, hipMemcpyHostToDevice, s));
    int64_t done = 0;
    const auto step = [&]() -> int32_t {
        if (exact) {
            if (nsup > 0) {                                          // the support rows' chains beside the SpMV
                RWR_HIP(hipEventRecord(g->ev_fork, s));
                RWR_HIP(hipStreamWaitEvent(s2, g->ev_fork, 0));
                hipLaunchKernelGGL(k_restart_fold, dim3((unsigned)nsup), dim3(WAVE), 0, s2, n, d_sup.p, d_vs.p, g->in_ptr.p,
                                   g->in_src.p, g->in_w.p, X, g->dangling.p, c1, d_fold.p);
                RWR_HIP(hipGetLastError());
                RWR_HIP(hipEventRecord(g->ev_join, s2));
            }
            sp.X = X, sp.Y = Y;
            launch_spmm(g, 1, 1, sp, s);
            if (nsup > 0) {
                RWR_HIP(hipStreamWaitEvent(s, g->ev_join, 0));
                hipLaunchKernelGGL(k_restart_scatter, dim3(cdiv((size_t)nsup, 256)), dim3(256), 0, s, nsup, d_sup.p, d_fold.p, Y);
            }
        } else {
            launch_restart_mass(g, X, c1, model_scalar(g), s);
            sp.X = X, sp.Y = Y;
            launch_spmm(g, 1, 1, sp, s);
            hipLaunchKernelGGL(k_add_restart_vec, dim3(cdiv((size_t)n, 256)), dim3(256), 0, s, Y, n, model_scalar(g), d_v.p);
        }
        RWR_HIP(hipGetLastError());
        std::swap(X, Y);
        return RWR_OK;
    };
    // checkConvergence (Model.cs:58-65, 110-115); exact: the reference's sequential sum of |rank - nextRank|, bit for bit
    // (same iteration count)
    RWR_TRY(run_walk(who, end, &done, step,
                     [&](double *dist) { return exact ? converge_exact(g, X, Y, dist) : converge_tree(g, X, Y, dist); }));
    RWR_HIP(hipMemcpyAsync(rank_out, X, sizeof(double) * n, hipMemcpyDeviceToHost, s));
    RWR_HIP(hipStreamSynchronize(s));
    if (iters_out) *iters_out = done;
    return RWR_OK;
}

static int32_t model_restart(rwr_graph *g, const double *v, const double *rank_in, double d, int32_t run_mode, double value,
                             bool one_step, double *rank_out, int64_t *iters_out, const char *who)
{
    return no_throw(who, [&] { return model_restart_body(g, v, rank_in, d, run_mode, value, one_step, rank_out, iters_out, who); });
}

int32_t model_run_restart(rwr_graph *g, const double *v, const double *rank_in, double d, int32_t run_mode, double value,
                          double *rank_out, int64_t *iters_out)
{
    return model_restart(g, v, rank_in, d, run_mode, value, false, rank_out, iters_out, "rwr_model_run_restart");
}

// one deliverRanks = a run of one step (only the given rank's signs matter for the SpMV's kernel choice)
int32_t model_deliver_restart(rwr_graph *g, const double *v, double d, const double *rank_in, double *next_out)
{
    return model_restart(g, v, rank_in, d, RWR_RUN_ITERATIONS, 1.0, true, next_out, nullptr, "rwr_model_deliver_restart");
}

}  // namespace rwr
