// Model.run / deliverRanks / checkConvergence (Model.cs:52-115) for one personalised or the global Model and for K
// personalised Models in one call, driven over GroupIter (iterate.h); the reductions that restart.hip (caller-set restart
// vectors) shares and GroupColumns, the column ends of a tile group of Models, which restart_batch.hip drives as well.
#include "iterate.h"
#include "seed_row.h"

#include <algorithm>
#include <cstdlib>

namespace rwr {

// ---- Model.run() / run(double) / global model (Model.cs:14-31, 52-66, 110-115) -------------------------------

// sum over i of |a_i - b_i|  (checkConvergence, Model.cs:110-115) or of the restart addends of the global model;
// deterministic two-level tree (the reference sums sequentially: tolerance-level difference)
constexpr int RED_GRID = 256;
__global__ __launch_bounds__(256) void k_l1_partial(const double *__restrict__ a, const double *__restrict__ b, int32_t n,
                                                    double *__restrict__ part)
{
    __shared__ double sh[256];
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double x = a[i], y = b[i];
        acc += (x > y) ? (x - y) : (y - x);                                  // Model.cs:113
    }
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
        if ((int)threadIdx.x < h) sh[threadIdx.x] += sh[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = sh[0];
}
__global__ __launch_bounds__(256) void k_absdiff(const double *__restrict__ a, const double *__restrict__ b, int32_t n,
                                                 double *__restrict__ d)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { const double x = a[i], y = b[i]; d[i] = (x > y) ? (x - y) : (y - x); }   // Math.Abs(rank - nextRank), Model.cs:113
}
__global__ __launch_bounds__(256) void k_rr_partial(const double *__restrict__ x, const uint8_t *__restrict__ dangling,
                                                    int32_t n, double c1, double *__restrict__ part)
{
    __shared__ double sh[256];
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double xi = x[i], rw = c1 * xi;
        acc += dangling[i] ? xi : (xi - rw);                                 // Model.cs:91 / :97
    }
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
        if ((int)threadIdx.x < h) sh[threadIdx.x] += sh[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = sh[0];
}
__global__ void k_sum_parts(const double *__restrict__ part, int nparts, double *__restrict__ out)
{
    double s = 0.0;
    for (int b = 0; b < nparts; ++b) s += part[b];
    *out = s;
}
__global__ void k_fill(double *__restrict__ x, int32_t n, double v)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] = v;
}
// global model: every node receives restart mass / n  (restart[r] = 1/n, Model.cs:29,92-93,96-97)
__global__ void k_add_restart_share(double *__restrict__ y, int32_t n, const double *__restrict__ total, double inv_n)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] += *total * inv_n;
}

// pieces of the global model and of checkConvergence that restart.hip (custom restart vectors) runs as well
static_assert(MODEL_RED_PARTS == RED_GRID, "engine.h: MODEL_RED_PARTS");
void launch_restart_mass(rwr_graph *g, const double *X, double c1, double *total, hipStream_t s)
{
    hipLaunchKernelGGL(k_rr_partial, dim3(RED_GRID), dim3(256), 0, s, X, g->dangling.p, g->n, c1, g->d_part.p);
    hipLaunchKernelGGL(k_sum_parts, dim3(1), dim3(1), 0, s, g->d_part.p, RED_GRID, total);
}
void launch_l1(rwr_graph *g, const double *a, const double *b, int32_t n, double *total, hipStream_t s)
{
    hipLaunchKernelGGL(k_l1_partial, dim3(RED_GRID), dim3(256), 0, s, a, b, n, g->d_part.p);
    hipLaunchKernelGGL(k_sum_parts, dim3(1), dim3(1), 0, s, g->d_part.p, RED_GRID, total);
}
void launch_absdiff(const double *a, const double *b, int32_t n, double *out, hipStream_t s)
{
    hipLaunchKernelGGL(k_absdiff, dim3(cdiv((size_t)n, 256)), dim3(256), 0, s, a, b, n, out);
}

// threshold runs that have not converged after this many steps fail (RWR_MAX_ITERS, read once per process)
int64_t model_max_iters()
{
    static const int64_t v = [] { const char *e = getenv("RWR_MAX_ITERS"); return e ? atoll(e) : (int64_t)1000000; }();
    return v;
}

RunEnd::RunEnd(int32_t run_mode, double value, int32_t n)
    : by_count(run_mode == RWR_RUN_ITERATIONS),
      // Model.cs:53: threshold = (1 / double.MaxValue) * n   (a subnormal-scale number: "until nothing changes")
      threshold(run_mode == RWR_RUN_DEFAULT_THRESHOLD ? (1 / 1.7976931348623157e308) * n : value),
      T(by_count ? (int64_t)value : model_max_iters()), max_iters(model_max_iters())
{
    if (T < 0) T = 0;
}

static int32_t read_distance(rwr_graph *g, double *dist)
{
    RWR_HIP(hipMemcpyAsync(dist, model_scalar(g), sizeof(double), hipMemcpyDeviceToHost, g->stream));
    RWR_HIP(hipStreamSynchronize(g->stream));
    return RWR_OK;
}
// the reference's sequential sum of |a[i] - b[i]|, reproduced bit for bit by the binade scan
// (d_evterm must exist for the scan's pointer arithmetic even though no link term is read)
int32_t converge_exact(rwr_graph *g, const double *a, const double *b, double *dist)
{
    RWR_TRY(g->cs_diff.ensure((size_t)g->n));
    RWR_TRY(g->d_evterm.ensure(1));
    launch_absdiff(a, b, g->n, g->cs_diff.p, g->stream);
    RWR_TRY(chain_scan_sum(g, g->cs_diff.p, model_scalar(g), g->stream));
    return read_distance(g, dist);
}
int32_t converge_tree(rwr_graph *g, const double *a, const double *b, double *dist)
{
    launch_l1(g, a, b, g->n, model_scalar(g), g->stream);
    return read_distance(g, dist);
}

// One step of the global model (Model.cs:14-31: restart = 1/n): every row receives the restart mass of every node,
// interleaved in node order in the reference; here: edge part in reference order + (tree-summed mass)/n.  Tolerance parity
// only.  g->d_seeds[0] holds -1 (no seed row to skip), g->d_part MODEL_RED_PARTS + 8 cells.
static int32_t global_model_step(rwr_graph *g, const double *X, double *Y, double c1, hipStream_t s)
{
    const int32_t n = g->n;
    launch_restart_mass(g, X, c1, model_scalar(g), s);
    SpmmArgs sp;
    sp.X = X, sp.Y = Y, sp.seeds = g->d_seeds.p, sp.c1 = c1;
    launch_spmm(g, 1, 1, sp, s);
    hipLaunchKernelGGL(k_add_restart_share, dim3(cdiv((size_t)n, 256)), dim3(256), 0, s, Y, n, model_scalar(g), 1.0 / n);
    RWR_HIP(hipGetLastError());
    return RWR_OK;
}

int32_t model_run(rwr_graph *g, int32_t seed, double d, int32_t run_mode, double value, double *rank_out,
                  int64_t *iters_out)
{
    const int32_t n = g->n;
    if (seed < -1 || seed >= n) {
        set_error("seed %d is outside [0, %d) (and is not -1 = global model)", seed, n);
        return RWR_E_RANGE;
    }
    // one model, one lane per row: the rank vector is contiguous
    const int G = 1;
    int TG = 1;
    RWR_TRY(ensure_workspace(g, G, 1, &TG));
    hipStream_t s = g->stream;
    Profile prof(g);
    const RunEnd end(run_mode, value, n);
    RWR_TRY(g->d_part.ensure(RED_GRID + 8));
    int64_t done = 0;
    double *Xf = nullptr;

    if (seed >= 0) {
        RWR_TRY(upload_seed_slots(g, &seed, 1, 1, nullptr));
        GroupIter gi(g, G, 1, g->d_seeds.p, g->d_evoff.p, d);
        RWR_TRY(gi.init());
        const auto step = [&] { return gi.step(plan_step(gi.cfg, gi.it, -1), prof); };   // deliverRanks + updateRanks
        const auto converge = [&](double *dist) -> int32_t {                             // checkConvergence (Model.cs:58-65)
            RWR_TRY(converge_exact(g, gi.Y, gi.X, dist));
            prof.reset();                                                                // (synchronised above: safe to recycle)
            return RWR_OK;
        };
        RWR_TRY(run_walk("rwr_model_run", end, &done, step, converge));
        Xf = gi.X;
    } else {
        RWR_TRY(ensure_in_w(g));   // (the global model runs the weighted kernels)
        double *X = g->X.p, *Y = g->Y.p;
        hipLaunchKernelGGL(k_fill, dim3(cdiv((size_t)n, 256)), dim3(256), 0, s, X, n, 1.0);   // rank = 1 (Model.cs:14-31)
        int32_t no_seed = -1;
        RWR_HIP(hipMemcpyAsync(g->d_seeds.p, &no_seed, sizeof(int32_t), hipMemcpyHostToDevice, s));
        const auto step = [&]() -> int32_t {
            RWR_TRY(global_model_step(g, X, Y, 1 - d, s));
            std::swap(X, Y);
            return RWR_OK;
        };
        RWR_TRY(run_walk("rwr_model_run", end, &done, step, [&](double *dist) { return converge_tree(g, Y, X, dist); }));
        Xf = X;
    }
    RWR_HIP(hipMemcpyAsync(rank_out, Xf, sizeof(double) * n, hipMemcpyDeviceToHost, s));
    RWR_HIP(hipStreamSynchronize(s));
    RWR_HIP(hipStreamSynchronize(g->stream2));
    if (prof.on) RWR_TRY(chain_scan_collect(g, s));
    if (iters_out) *iters_out = done;
    return RWR_OK;
}

// One Model.deliverRanks (Model.cs:76-100) on a rank vector supplied by the caller: backs the public step-by-step API
// (deliverRanks / updateRanks / checkConvergence, Model.cs:76,103,110) for hosts that drive the loop themselves.
int32_t model_deliver(rwr_graph *g, int32_t seed, double d, const double *rank_in, double *next_out)
{
    const int32_t n = g->n;
    if (seed < -1 || seed >= n) {
        set_error("seed %d is outside [0, %d) (and is not -1 = global model)", seed, n);
        return RWR_E_RANGE;
    }
    int TG = 1;
    RWR_TRY(ensure_workspace(g, 1, 1, &TG));
    hipStream_t s = g->stream;
    bool nonneg = true;
    for (int32_t i = 0; i < n; ++i)
        if (!(rank_in[i] >= 0.0)) { nonneg = false; break; }
    RWR_HIP(hipMemcpyAsync(g->X.p, rank_in, sizeof(double) * n, hipMemcpyHostToDevice, s));
    double *out = nullptr;
    if (seed >= 0) {
        RWR_TRY(upload_seed_slots(g, &seed, 1, 1, nullptr));
        Profile prof(g);
        GroupIter gi(g, 1, 1, g->d_seeds.p, g->d_evoff.p, d);
        RWR_TRY(gi.init(false, nonneg));
        RWR_TRY(gi.step(plan_step(gi.cfg, 0, -1), prof));
        RWR_HIP(hipStreamSynchronize(s));
        RWR_HIP(hipStreamSynchronize(g->stream2));
        if (prof.on) RWR_TRY(chain_scan_collect(g, s));
        out = gi.X;                                   // (step() swapped: X holds nextRank)
    } else {
        RWR_TRY(ensure_in_w(g));
        RWR_TRY(g->d_part.ensure(RED_GRID + 8));
        int32_t no_seed = -1;
        RWR_TRY(g->d_seeds.ensure(1));
        RWR_HIP(hipMemcpyAsync(g->d_seeds.p, &no_seed, sizeof(int32_t), hipMemcpyHostToDevice, s));
        RWR_TRY(global_model_step(g, g->X.p, g->Y.p, 1 - d, s));
        out = g->Y.p;
    }
    RWR_HIP(hipMemcpyAsync(next_out, out, sizeof(double) * n, hipMemcpyDeviceToHost, s));
    RWR_HIP(hipStreamSynchronize(s));
    return RWR_OK;
}

// ---- K personalised Models in one call (rwr_model_run_batch) -------------------------------------------

// |rank - nextRank| of every element of a tile group's [tile][n][G] matrices (Model.cs:113): the addends of the G-wide
// checkConvergence scan
__global__ __launch_bounds__(256) void k_absdiff_mat(const double *__restrict__ a, const double *__restrict__ b, int64_t elems,
                                                     double *__restrict__ d)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < elems; i += (int64_t)gridDim.x * blockDim.x) {
        const double x = a[i], y = b[i];
        d[i] = (x > y) ? (x - y) : (y - x);
    }
}

// Columns of a tile group's rank matrix X[tile][n][G] into row-major staging rows: slot (tile, k) with row_of[tile * G + k] =
// j >= 0 goes to out[j * n ...].  A workgroup takes EX_ELEMS consecutive elements of one tile (EX_ELEMS / G whole rows),
// reads them coalesced into LDS (row stride G + 1: a column walk hits distinct banks) and writes each selected column's
// piece as one contiguous run.
constexpr int EX_ELEMS = 2048;
template <int G>
__global__ __launch_bounds__(256) void k_extract_cols(int32_t n, const double *__restrict__ X, const int32_t *__restrict__ row_of,
                                                      double *__restrict__ out)
{
    constexpr int ROWS = EX_ELEMS / G;
    __shared__ double t[ROWS * (G + 1)];
    const int tile = blockIdx.y;
    const int32_t *sel = row_of + (size_t)tile * G;
    bool any = false;
    for (int k = 0; k < G; ++k) any = any || sel[k] >= 0;
    if (!any) return;                                        // no column of this tile is wanted now (uniform per workgroup)
    const int64_t r0 = (int64_t)blockIdx.x * ROWS;
    const int nr = (int)((int64_t)n - r0 < ROWS ? (int64_t)n - r0 : ROWS);
    const double *x = X + (size_t)tile * (size_t)n * G + (size_t)r0 * G;
    for (int q = threadIdx.x; q < nr * G; q += 256) t[(q / G) * (G + 1) + (q % G)] = x[q];
    __syncthreads();
    for (int q = threadIdx.x; q < G * ROWS; q += 256) {
        const int k = q / ROWS, r = q % ROWS;
        const int32_t j = sel[k];
        if (j >= 0 && r < nr) out[(size_t)j * (size_t)n + (size_t)(r0 + r)] = t[r * (G + 1) + k];
    }
}

static void launch_absdiff_mat(const double *a, const double *b, size_t elems, double *out, hipStream_t s)
{
    hipLaunchKernelGGL(k_absdiff_mat, dim3(std::min<size_t>(cdiv(elems, 256), 16384)), dim3(256), 0, s, a, b, (int64_t)elems, out);
}
static void launch_extract_cols(rwr_graph *g, int G, int tg, const double *X, const int32_t *row_of, double *out, hipStream_t s)
{
    RWR_DISPATCH_G(G, hipLaunchKernelGGL(k_extract_cols<GG>, dim3(cdiv((size_t)g->n, EX_ELEMS / GG), (unsigned)tg), dim3(256), 0, s,
                                         g->n, X, row_of, out));
}

int32_t GroupColumns::emit(int64_t steps, const double *X)
{
    const size_t n = (size_t)g->n;
    hipStream_t s = g->stream;
    if (ends.leaving(steps, dist.data(), row_of.data(), iters_out) == 0) return RWR_OK;
    RWR_HIP(hipMemcpyAsync(g->mb_row.p, row_of.data(), ends.nslots * sizeof(int32_t), hipMemcpyHostToDevice, s));
    hipEvent_t a; RWR_TRY(prof.record(a, s));
    launch_extract_cols(g, G, tg, X, g->mb_row.p, g->cs_diff.p, s);
    RWR_HIP(hipGetLastError());
    RWR_TRY(prof.end(prof.rank, a, s));
    for (size_t q = 0; q < ends.nslots; ++q)
        if (row_of[q] >= 0)
            RWR_HIP(hipMemcpyAsync(rank_out + (size_t)ends.slot_k[q] * n, g->cs_diff.p + (size_t)row_of[q] * n, sizeof(double) * n,
                                   hipMemcpyDeviceToHost, s));
    RWR_HIP(hipStreamSynchronize(s));
    return prof.fold(g);
}

int32_t GroupColumns::measure(hipEvent_t i0, const double *Y, const double *X)
{
    hipStream_t s = g->stream;
    launch_absdiff_mat(Y, X, ends.nslots * (size_t)g->n, g->cs_diff.p, s);
    RWR_TRY(chain_scan_sum_cols(g, G, tg, g->cs_diff.p, evoff, g->cs_sums.p, s));
    RWR_TRY(prof.end(prof.iter, i0, s));
    RWR_HIP(hipMemcpyAsync(dist.data(), g->cs_sums.p, ends.nslots * sizeof(double), hipMemcpyDeviceToHost, s));
    RWR_HIP(hipStreamSynchronize(s));
    return prof.fold(g);
}

int32_t finish_model_batch(rwr_graph *g, Profile &prof, int G, int TG, double t_begin)
{
    RWR_HIP(hipStreamSynchronize(g->stream));
    RWR_HIP(hipStreamSynchronize(g->stream2));
    RWR_TRY(prof.fold(g));
    if (prof.on) RWR_TRY(chain_scan_collect(g, g->stream));
    g->stats.tile_seeds = G;
    g->stats.tile_group = TG;
    g->stats.total_wall_ms += now_ms() - t_begin;
    return RWR_OK;
}

// Tile group by tile group: GroupIter (no frontier-list steps, no row lists: every step writes every row of X), then each
// real slot's column goes to its caller row -- after step T (iteration mode) or after the step at which its own
// checkConvergence holds (threshold modes; the sums of all G * tg columns come back with one synchronisation per step).
static int32_t model_run_batch_body(rwr_graph *g, const int32_t *seeds, int32_t K, double d, int32_t run_mode, double value,
                                    double *rank_out, int64_t *iters_out)
{
    const double t_begin = now_ms();
    const int32_t n = g->n;
    // one Model, or a graph / damping factor outside the domain of the batched kernels (negative ranks: the frontier
    // kernels and the binade scan step aside, and the G > 1 step was never checked there): rwr_model_run per seed.
    // Its statistics are those of K rwr_model_run calls (tile_seeds / tile_group untouched) plus this call's wall time.
    if (K == 1 || !g->nonneg || !(d >= 0.0 && d <= 1.0)) {
        for (int32_t k = 0; k < K; ++k)
            RWR_TRY(model_run(g, seeds[k], d, run_mode, value, rank_out + (size_t)k * n, iters_out ? iters_out + k : nullptr));
        g->stats.total_wall_ms += now_ms() - t_begin;
        return RWR_OK;
    }
    const RunEnd end(run_mode, value, n);
    const int G = resolve_G(g, K);
    int TG = 1;
    RWR_TRY(ensure_workspace(g, G, K, &TG, 1));             // + cs_diff: differences, then staging of the extracted columns
    const int ntiles = (int)cdiv((size_t)K, (size_t)G);
    std::vector<int32_t> slot_k;
    RWR_TRY(upload_seed_slots(g, seeds, K, G, &slot_k));
    RWR_TRY(g->cs_sums.ensure((size_t)TG * G));
    RWR_TRY(g->mb_row.ensure((size_t)TG * G));
    hipStream_t s = g->stream;
    StreamsIdle idle{g};                                     // (also when a step fails or RWR_MAX_ITERS runs out)
    Profile prof(g);                                         // (column extraction counts as ranking time)
    for (int t0 = 0; t0 < ntiles; t0 += TG) {
        const int tg = (ntiles - t0 < TG) ? (ntiles - t0) : TG;
        const size_t q0 = (size_t)t0 * G;
        GroupColumns cols(g, G, tg, slot_k.data() + q0, g->d_evoff.p + q0, end, rank_out, iters_out, prof);
        GroupIter gi(g, G, tg, g->d_seeds.p + q0, cols.evoff, d);
        RWR_TRY(gi.init(true, true, /*ranking_only=*/false));
        if (!end.by_count) RWR_TRY(chain_scan_sum_cols_prepare(g, G, tg, s));
        int64_t steps = 0;
        for (;;) {
            if (cols.ends.due(steps)) {
                RWR_TRY(cols.emit(steps, gi.X));
                if (cols.ends.done()) break;
            }
            if (steps == end.T) {                            // RWR_MAX_ITERS steps made: the later groups do not run
                set_error("rwr_model_run_batch: no convergence within %lld iterations (RWR_MAX_ITERS)", (long long)end.max_iters);
                return RWR_E_UNSUPPORTED;
            }
            hipEvent_t i0; RWR_TRY(prof.record(i0, s));
            RWR_TRY(gi.step(plan_step(gi.cfg, steps, end.by_count ? end.T : -1), prof));   // deliverRanks + updateRanks
            ++steps;
            RWR_TRY(end.by_count ? prof.end(prof.iter, i0, s) : cols.measure(i0, gi.Y, gi.X));
        }
        cols.count(steps, gi.dense_steps);
    }
    return finish_model_batch(g, prof, G, TG, t_begin);
}

int32_t model_run_batch(rwr_graph *g, const int32_t *seeds, int32_t K, double d, int32_t run_mode, double value,
                        double *rank_out, int64_t *iters_out)
{
    return no_throw("rwr_model_run_batch",
                    [&] { return model_run_batch_body(g, seeds, K, d, run_mode, value, rank_out, iters_out); });
}

}  // namespace rwr
