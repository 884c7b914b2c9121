// Row-partitioned mode (include/rwr.h: rwr_part_*): each rank holds the out-links of a slab of rows and computes its partial
// y over all n rows plus its slab's restart mass; the caller sums the partials over the ranks.  The SpMM and the frontier
// marking are the batched step's kernels (iterate.h); the exclusion and the ranking are rank.hip's.
#include "iterate.h"

namespace rwr {

constexpr int RP_GRID = 512;
constexpr int RP_BLOCK = 256;

// restart mass of the slab's rows only: r[k] = sum over i in [lo, hi) of (dangling_i ? x_i : x_i - (1-d) x_i)
template <int G>
__global__ __launch_bounds__(RP_BLOCK) void k_slab_restart_partial(int32_t lo, int32_t hi,
                                                                   const uint8_t *__restrict__ dangling,
                                                                   const double *__restrict__ x,
                                                                   double *__restrict__ part, double c1)
{
    constexpr int RL = RP_BLOCK / G;
    __shared__ double sh[RP_BLOCK];
    const int k = threadIdx.x % G, rl = threadIdx.x / G;
    double acc = 0.0;
    for (int64_t i = (int64_t)lo + (int64_t)blockIdx.x * RL + rl; i < hi; i += (int64_t)gridDim.x * RL) {
        const double xi = x[(size_t)i * G + k];
        const double rw = c1 * xi;
        acc += dangling[i] ? xi : (xi - rw);
    }
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int half = RL / 2; half >= 1; half >>= 1) {
        if (rl < half) sh[threadIdx.x] += sh[threadIdx.x + half * G];
        __syncthreads();
    }
    if (rl == 0) part[(size_t)blockIdx.x * G + k] = sh[k];
}
__global__ void k_slab_restart_final(int G, int nblk, const double *__restrict__ part, double *__restrict__ r)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= G) return;
    double R = 0.0;
    for (int b = 0; b < nblk; ++b) R += part[(size_t)b * G + k];
    r[k] = R;
}
__global__ void k_part_add_restart(int G, double *__restrict__ y, const double *__restrict__ r,
                                   const int32_t *__restrict__ seeds)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= G) return;
    const int32_t s = seeds[k];
    if (s >= 0) y[(size_t)s * G + k] += r[k];
}

int32_t part_begin(rwr_graph *g, int32_t lo, int32_t hi, const int32_t *seeds, int32_t K, double d, double *x,
                   int32_t *G_out)
{
    const int32_t n = g->n;
    if (lo < 0 || hi > n || lo > hi) { set_error("rwr_part_begin: bad slab [%d, %d)", lo, hi); return RWR_E_RANGE; }
    if (K < 1 || K > 64) { set_error("rwr_part_begin: K must be 1..64 in row-partitioned mode"); return RWR_E_UNSUPPORTED; }
    for (int32_t k = 0; k < K; ++k)
        if (seeds[k] < 0 || seeds[k] >= n) { set_error("seed %d is outside [0, %d)", seeds[k], n); return RWR_E_RANGE; }
    int G = 1;
    while (G < K) G <<= 1;
    // value-free graphs (every BASELINE configuration): the slab step forms z = ((1-d) x) * w_src for the slab's rows and
    // the kernels gather z -- 4 instead of 12 matrix bytes per entry, and no in_w (2 GB per rank at 1/8 of the 1 G-like
    // graph) is ever materialised; other graphs run the weighted kernels on the caller's rank matrix
    if (g->vf) RWR_TRY(g->Z0.ensure((size_t)(hi - lo > 0 ? hi - lo : 1) * (size_t)G));
    else RWR_TRY(ensure_in_w(g));
    g->part_lo = lo; g->part_hi = hi; g->part_G = G; g->part_K = K; g->part_c1 = 1 - d;
    g->part_steps = 0;
    if (g->vf && g->nonneg && G >= 8) RWR_TRY(g->d_nz.ensure(2 * (((size_t)n + 31) / 32)));   // frontier of the first steps
    g->part_seeds.assign((size_t)G, -1);
    for (int32_t k = 0; k < K; ++k) g->part_seeds[k] = seeds[k];
    RWR_TRY(g->d_seeds.ensure(G));
    RWR_TRY(g->d_part.ensure((size_t)RP_GRID * G + G));
    RWR_HIP(hipMemcpy(g->d_seeds.p, g->part_seeds.data(), G * sizeof(int32_t), hipMemcpyHostToDevice));
    hipStream_t s = g->stream;
    RWR_HIP(hipMemsetAsync(x, 0, (size_t)n * G * sizeof(double), s));
    launch_init_seeds(g, G, 1, x, g->d_seeds.p, nullptr, nullptr, 0.0, s);
    RWR_HIP(hipGetLastError());
    RWR_HIP(hipStreamSynchronize(s));
    if (G_out) *G_out = G;
    return RWR_OK;
}

// y = (1-d) P_slab^T x over all n rows.  Value-free graphs: z of the slab's rows first (the in-lists of the slab graph
// hold in-slab sources only, so the kernels' gathers z[source * G + k] never leave [lo, hi): the buffer holds just the
// slab, addressed through a base pointer shifted by lo rows)
static int32_t part_spmm(rwr_graph *g, const double *x, double *y, hipStream_t s)
{
    const int G = g->part_G;
    const double c1 = g->part_c1;
    if (g->vf) {
        const int64_t rows = (int64_t)g->part_hi - g->part_lo;
        if (rows > 0 && (!g->Z0.p || g->Z0.count < (size_t)rows * G)) { set_error("rwr_part_step: call rwr_part_begin"); return RWR_E_INVALID; }
        const int64_t elems = rows * G;
        const double *zin = g->Z0.p - (size_t)g->part_lo * G;
        // the first steps after rwr_part_begin (the ranks are still concentrated around the seeds): mark the slab's non-zero rows
        // and -- the first two steps -- the destination rows their out-links reach, and let the SpMM skip every other row and
        // every gather of an all-zero source row: what the seed path does in its first iterations (GroupIter::init); exact
        // for ANY rank matrix (a skipped addend is +0.0), the step counter only decides whether the marking is worth its cost
        static const int part_act_env = [] { const char *e = RWR_TUNE_ENV("RWR_PART_ACT_STEPS"); return e ? atoi(e) : 2; }();
        static const int part_nz_env = [] { const char *e = RWR_TUNE_ENV("RWR_PART_NZ_STEPS"); return e ? atoi(e) : 4; }();
        const size_t nzw = ((size_t)g->n + 31) / 32;
        const bool frontier = g->part_steps < part_nz_env && g->nonneg && G >= 8 && rows > 0 && g->d_nz.p && g->d_nz.count >= 2 * nzw;
        const bool mark = frontier && g->part_steps < part_act_env;      // (later steps: only the per-entry probe of the sources)
        ++g->part_steps;
        SpmmArgs sp;
        sp.X = x, sp.Y = y, sp.seeds = g->d_seeds.p, sp.c1 = c1, sp.Zin = zin;
        if (frontier) {
            uint32_t *nz = g->d_nz.p, *act = g->d_nz.p + nzw;
            RWR_HIP(hipMemsetAsync(nz, 0, (mark ? 2 : 1) * nzw * sizeof(uint32_t), s));
            launch_make_z_nz(g, g->part_lo, g->part_hi, G, x, g->Z0.p, c1, nz, s);
            if (mark) launch_mark_active(g, 0, 1, nz, act, nullptr, nullptr, nullptr, s);
            sp.nz_in = nz, sp.act = mark ? act : nullptr;
        } else if (elems > 0) {
            launch_make_z(elems, G, x + (size_t)g->part_lo * G, g->Z0.p, g->w_src.p + g->part_lo, c1, s);
        }
        launch_spmm(g, G, 1, sp, s);
    } else {
        if (!g->in_w.p) { set_error("rwr_part_step: call rwr_part_begin"); return RWR_E_INVALID; }
        SpmmArgs sp;
        sp.X = x, sp.Y = y, sp.seeds = g->d_seeds.p, sp.c1 = c1;
        launch_spmm(g, G, 1, sp, s);
    }
    return RWR_OK;
}

int32_t part_local_step(rwr_graph *g, const double *x, double *y, double *r)
{
    const int G = g->part_G;
    if (G == 0) { set_error("rwr_part_local_step: rwr_part_begin has not been called"); return RWR_E_INVALID; }
    hipStream_t s = g->stream;
    const double c1 = g->part_c1;
    RWR_DISPATCH_G(G, hipLaunchKernelGGL(k_slab_restart_partial<GG>, dim3(RP_GRID), dim3(RP_BLOCK), 0, s, g->part_lo,
                                         g->part_hi, g->dangling.p, x, g->d_part.p, c1));
    hipLaunchKernelGGL(k_slab_restart_final, dim3(1), dim3(64), 0, s, G, RP_GRID, g->d_part.p, r);
    // the graph holds only this slab's out-links, so the in-lists contain only in-slab sources
    RWR_TRY(part_spmm(g, x, y, s));
    RWR_HIP(hipGetLastError());
    RWR_HIP(hipStreamSynchronize(s));
    return RWR_OK;
}

// One whole local step on the caller's stream, no host synchronisation: partial y over all rows, plus this slab's restart
// mass at the seeds' rows -- the sum over the ranks of y is then the next rank matrix (include/rwr.h: rwr_part_step).
int32_t part_step(rwr_graph *g, const double *x, double *y, hipStream_t stream)
{
    const int G = g->part_G;
    if (G == 0) { set_error("rwr_part_step: rwr_part_begin has not been called"); return RWR_E_INVALID; }
    hipStream_t s = stream;                              // exactly the caller's stream (NULL = the device's default stream)
    const double c1 = g->part_c1;
    double *r = g->d_part.p + (size_t)RP_GRID * G;       // (behind the per-block partials)
    RWR_DISPATCH_G(G, hipLaunchKernelGGL(k_slab_restart_partial<GG>, dim3(RP_GRID), dim3(RP_BLOCK), 0, s, g->part_lo,
                                         g->part_hi, g->dangling.p, x, g->d_part.p, c1));
    hipLaunchKernelGGL(k_slab_restart_final, dim3(1), dim3(64), 0, s, G, RP_GRID, g->d_part.p, r);
    RWR_TRY(part_spmm(g, x, y, s));
    hipLaunchKernelGGL(k_part_add_restart, dim3(1), dim3(64), 0, s, G, y, r, g->d_seeds.p);
    RWR_HIP(hipGetLastError());
    return RWR_OK;
}

int32_t part_finish_step(rwr_graph *g, double *y, const double *r)
{
    const int G = g->part_G;
    if (G == 0) { set_error("rwr_part_finish_step: rwr_part_begin has not been called"); return RWR_E_INVALID; }
    hipLaunchKernelGGL(k_part_add_restart, dim3(1), dim3(64), 0, g->stream, G, y, r, g->d_seeds.p);
    RWR_HIP(hipGetLastError());
    RWR_HIP(hipStreamSynchronize(g->stream));
    return RWR_OK;
}

int32_t part_rank(rwr_graph *g, double *x, int32_t top_n, int64_t *ids, double *scores, int32_t *counts)
{
    const int G = g->part_G, K = g->part_K;
    if (G == 0) { set_error("rwr_part_rank: rwr_part_begin has not been called"); return RWR_E_INVALID; }
    if (top_n < 1 || top_n > rank_select_max_k()) {
        set_error("rwr_part_rank: top_n must be 1..%d", rank_select_max_k());
        return RWR_E_UNSUPPORTED;
    }
    hipStream_t s = g->stream;
    // only the owner of a seed's row has its raw LIKE links (exclusion list): rank those, report -1 for the rest
    std::vector<int32_t> own((size_t)G, -1), slot_k((size_t)G, -1);
    for (int k = 0; k < K; ++k)
        if (g->part_seeds[k] >= g->part_lo && g->part_seeds[k] < g->part_hi) { own[k] = g->part_seeds[k]; slot_k[k] = k; }
    DevBuf<int32_t> d_own;
    RWR_TRY(d_own.alloc(G));
    return idle_on_error(s, [&]() -> int32_t {
        RWR_TRY(g->d_slot_k.ensure(G));
        RWR_HIP(hipMemcpy(d_own.p, own.data(), G * sizeof(int32_t), hipMemcpyHostToDevice));
        RWR_HIP(hipMemcpy(g->d_slot_k.p, slot_k.data(), G * sizeof(int32_t), hipMemcpyHostToDevice));
        const size_t out_elems = (size_t)G * top_n;
        RWR_TRY(g->d_out_id.ensure(out_elems));
        RWR_TRY(g->d_out_score.ensure(out_elems));
        RWR_TRY(g->d_counts.ensure(G));
        RWR_HIP(hipMemsetAsync(g->d_out_id.p, 0, out_elems * sizeof(int64_t), s));
        RWR_HIP(hipMemsetAsync(g->d_out_score.p, 0, out_elems * sizeof(double), s));
        RWR_HIP(hipMemsetAsync(g->d_counts.p, 0, G * sizeof(int32_t), s));
        launch_exclude(g, G, 1, x, d_own.p, s);
        RWR_TRY(rank_group_select(g, G, 1, g->d_slot_k.p, top_n, x, d_own.p, s));
        std::vector<int32_t> hc((size_t)G);
        RWR_HIP(hipMemcpyAsync(hc.data(), g->d_counts.p, G * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        RWR_HIP(hipMemcpyAsync(ids, g->d_out_id.p, (size_t)K * top_n * sizeof(int64_t), hipMemcpyDeviceToHost, s));
        RWR_HIP(hipMemcpyAsync(scores, g->d_out_score.p, (size_t)K * top_n * sizeof(double), hipMemcpyDeviceToHost, s));
        RWR_HIP(hipStreamSynchronize(s));
        for (int k = 0; k < K; ++k) counts[k] = own[k] >= 0 ? hc[k] : -1;
        return RWR_OK;
    });
}

}  // namespace rwr
