// Ranking inside a batch's last step.  The select (rank.hip) has ranked the head -- the first H rows of
// tail_rows[0] -- exactly: row orow of the result tables holds each seed's top_n of the head and its count.  Their top_n-th
// scores become the thresholds the rest of the step selects by (k_spmm_select, iterate.hip), a float bound prunes the body rows
// no seed of a tile can still need (rank_bound.h), and one merge per seed sorts the head's list with the candidates.
#include "iterate.h"
#include "rank_bound.h"
#include "rank_keys.h"

namespace rwr {

static_assert(FUSED_SORT_SLOTS == SEL_SLOTS, "rank_plan.h sizes the candidate capacity by the merge's sort slots");

// k_sel_tau: the threshold the rest of the step selects by -- the score of the head's top_n-th entry, a lower bound of the
// final top_n-th score, or 0 (every score qualifies) when the head gave fewer than top_n; and the cleared append cursor.
__global__ void k_sel_tau(int nseg, int32_t top_n, const int32_t *__restrict__ slot_k, const int32_t *__restrict__ out_counts,
                          const double *__restrict__ out_score, double *__restrict__ tau, int32_t *__restrict__ cursor)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nseg) return;
    const int32_t orow = slot_k[q];
    double t = 0.0;
    if (orow >= 0 && out_counts[orow] >= top_n) t = out_score[(size_t)orow * top_n + (top_n - 1)];
    tau[q] = t;
    cursor[q] = 0;
}

// k_sel_merge, one block per slot: the head's entries and the rows k_spmm_select appended -- less the seed's raw LIKE links,
// read exactly as k_exclude reads them, in whatever order the list holds them -- sorted by (score desc, id desc); the first
// top_n and the count go out.  The append order differs from run to run; the keys are unique, so the result does not.
constexpr int MERGE_LIKES = 256;
__global__ __launch_bounds__(256) void k_sel_merge(const int32_t *__restrict__ slot_k, const int32_t *__restrict__ seeds,
                                                   int32_t top_n, const int32_t *__restrict__ cursor,
                                                   const RowScore *__restrict__ body, int32_t cap, int32_t stride,
                                                   const int64_t *__restrict__ rowptr, const int32_t *__restrict__ dst,
                                                   const uint8_t *__restrict__ etype, const int64_t *__restrict__ node_id,
                                                   int64_t *__restrict__ out_id, double *__restrict__ out_score,
                                                   int32_t *__restrict__ out_counts)
{
    extern __shared__ SelCand sc[];
    __shared__ int32_t likes[MERGE_LIKES];
    __shared__ int n_excl;
    const int seg = blockIdx.x, tid = threadIdx.x;
    const int32_t orow = slot_k[seg];
    const int32_t seed = seeds[seg];
    if (orow < 0 || seed < 0) return;
    int hc = out_counts[orow];
    if (hc > top_n) hc = top_n;
    int bc = cursor[seg];
    if (bc > cap) bc = cap;
    if (bc == 0) return;                         // nothing beyond the head: its list stands
    const int total = hc + bc;                   // <= top_n + cap <= SEL_SLOTS
    int N2 = 1;
    while (N2 < total) N2 <<= 1;
    if (tid == 0) n_excl = 0;
    const RowScore *b = body + (size_t)seg * (size_t)stride;
    for (int i = tid; i < N2; i += blockDim.x) {
        SelCand c{0ull, 0ull};
        if (i < hc) {
            c.hi = f64_orderable(out_score[(size_t)orow * top_n + i]);
            c.lo = i64_orderable(out_id[(size_t)orow * top_n + i]);
        } else if (i < total) {
            const RowScore r = b[i - hc];
            c.hi = f64_orderable(r.score);       // (>= 2^63: scores are >= +0.0)
            c.lo = (uint64_t)(uint32_t)r.row;    // the row, until the exclusion is through
        }
        sc[i] = c;
    }
    __syncthreads();
    // Recommender.cs:20-24,29: the seed's raw LIKE links are no candidates
    const int64_t p0 = rowptr[seed], p1 = rowptr[seed + 1];
    for (int64_t pb = p0; pb < p1; pb += MERGE_LIKES) {
        const int64_t p = pb + tid;
        if (tid < MERGE_LIKES) likes[tid] = (p < p1 && etype[p] == RWR_EDGE_LIKE) ? dst[p] : -1;
        __syncthreads();
        const int nl = (p1 - pb < MERGE_LIKES) ? (int)(p1 - pb) : MERGE_LIKES;
        for (int i = hc + tid; i < total; i += blockDim.x) {
            const SelCand c = sc[i];
            if (c.hi == 0ull) continue;          // excluded already (a link listed twice)
            const int32_t row = (int32_t)c.lo;
            bool hit = false;
            for (int l = 0; l < nl; ++l) hit = hit || likes[l] == row;
            if (hit) {
                sc[i] = SelCand{0ull, 0ull};
                atomicAdd(&n_excl, 1);
            }
        }
        __syncthreads();
    }
    for (int i = hc + tid; i < total; i += blockDim.x)
        if (sc[i].hi != 0ull) sc[i].lo = i64_orderable(node_id[(int32_t)sc[i].lo]);
    __syncthreads();
    sel_sort_emit(sc, N2, total - n_excl, orow, top_n, out_id, out_score, out_counts);
}

// The second half of the ranking inside the last step; the workspace of a group's tau, cursors, overflow flag
// and candidate buffers (fused_capacity() per slot, rank_plan.h), the threshold after the head's select (fills *sink), the
// merge after the selecting launch
static int32_t rank_fused_prepare(rwr_graph *g, int G, int tg, const int32_t *d_slot_k, int32_t top_n, SelSink *sink,
                                  hipStream_t s)
{
    const size_t nseg = (size_t)tg * G;
    const int cap = fused_capacity(top_n, rank_knobs());
    const size_t tau_bytes = nseg * sizeof(double), cur_bytes = ((nseg + 2) * sizeof(int32_t) + 15) & ~(size_t)15;
    RWR_TRY(g->fused_ws.ensure(tau_bytes + cur_bytes + nseg * (size_t)cap * sizeof(RowScore) + 64));
    sink->tau = (const double *)g->fused_ws.p;
    sink->cursor = (int32_t *)(g->fused_ws.p + tau_bytes);
    sink->overflow = sink->cursor + nseg;
    sink->cand = (RowScore *)(g->fused_ws.p + tau_bytes + cur_bytes);
    sink->cap = cap, sink->stride = cap;
    RWR_HIP(hipMemsetAsync(sink->overflow, 0, sizeof(int32_t), s));
    hipLaunchKernelGGL(k_sel_tau, dim3(cdiv(nseg, 64)), dim3(64), 0, s, (int)nseg, top_n, d_slot_k, g->d_counts.p, g->d_out_score.p,
                       (double *)g->fused_ws.p, sink->cursor);
    RWR_HIP(hipGetLastError());
    return RWR_OK;
}
static int32_t rank_fused_merge(rwr_graph *g, int G, int tg, const int32_t *d_slot_k, const int32_t *d_seeds, int32_t top_n,
                                const SelSink &sink, hipStream_t s)
{
    (void)hipFuncSetAttribute((const void *)k_sel_merge, hipFuncAttributeMaxDynamicSharedMemorySize,
                              SEL_SLOTS * (int)sizeof(SelCand));
    hipLaunchKernelGGL(k_sel_merge, dim3((unsigned)(tg * G)), dim3(256), SEL_SLOTS * sizeof(SelCand), s, d_slot_k, d_seeds, top_n,
                       sink.cursor, sink.cand, sink.cap, sink.stride, g->rowptr.p, g->dst.p, g->etype.p, g->node_id.p,
                       g->d_out_id.p, g->d_out_score.p, g->d_counts.p);
    RWR_HIP(hipGetLastError());
    return RWR_OK;
}

// ---------------------------------------------------------------------------------------
// Pruning the body of the last step (rank_bound.h).  k_spmm_select gathers a G x 8-byte row of z per in-link to
// learn that nearly every body row stays below every threshold of the tile.  Once k_sel_tau has the thresholds, the bound
//     m[u][tile] = max over the tile's real slots of z[u][slot] / tau[slot], rounded up to float
// settles that with one float per in-link: a row whose sum of m over its in-list stays below 1 reaches tau for no seed.
// The tables are laid out [block of BOUND_W tiles][source row][BOUND_W], so that ONE 128-byte line per in-link serves 32 tiles:
// lane = tile, and the bound pass is the chunked SpMM's walk once more, in float, over 1/32 of the lines, once for all tiles.
// Value-free path only (z >= 0, no per-link weight).
// ---------------------------------------------------------------------------------------
constexpr int BOUND_W = 32;

// noprune[tile] = 1: a real slot of the tile has threshold 0 -- every score qualifies, rows without in-links included
__global__ void k_sel_bound_flags(int tg, int G, const int32_t *__restrict__ seeds, const double *__restrict__ tau,
                                  int32_t *__restrict__ noprune)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= tg) return;
    int32_t f = 0;
    for (int k = 0; k < G; ++k)
        if (seeds[t * G + k] >= 0 && !(tau[t * G + k] > 0.0)) f = 1;
    noprune[t] = f;
}

// source rows [lo, hi) of the in-links of rows[0 .. nrows): range[0] = min, range[1] = max (once per graph and head size)
__global__ __launch_bounds__(256) void k_sel_bound_range(const int64_t *__restrict__ in_ptr, const int32_t *__restrict__ in_src,
                                                         const int32_t *__restrict__ rows, int32_t nrows, int32_t *__restrict__ range)
{
    int32_t lo = INT32_MAX, hi = -1;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < nrows; r += (int64_t)gridDim.x * blockDim.x) {
        const int32_t j = rows[r];
        for (int64_t p = in_ptr[j], e = in_ptr[j + 1]; p < e; ++p) {
            const int32_t u = in_src[p];
            lo = u < lo ? u : lo;
            hi = u > hi ? u : hi;
        }
    }
    for (int sh = WAVE / 2; sh > 0; sh >>= 1) {
        const int32_t l2 = __shfl_xor(lo, sh), h2 = __shfl_xor(hi, sh);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
    }
    if ((threadIdx.x & (WAVE - 1)) == 0 && hi >= 0) {
        atomicMin(&range[0], lo);
        atomicMax(&range[1], hi);
    }
}

// m of the source rows [src_lo, src_lo + nsrc) for every tile: a lane group reads the row's G values of one tile (one
// coalesced load), divides by the slots' thresholds, rounds up and takes the maximum; padded slots and slots with threshold 0
// (their tile is flagged noprune) contribute nothing; the lanes of tiles past tg hold 0.  A workgroup writes whole 128-byte lines.
template <int G>
__global__ __launch_bounds__(256) void k_sel_bound_table(int32_t n, int tg, int32_t src_lo, int32_t nsrc,
                                                         const double *__restrict__ Z, const int32_t *__restrict__ seeds,
                                                         const double *__restrict__ tau, float *__restrict__ m)
{
    constexpr int GROUPS = 256 / G, NT = BOUND_W / GROUPS;   // lane groups of the workgroup, tiles per group
    const int k = threadIdx.x % G, grp = threadIdx.x / G;
    const int blk = blockIdx.y;
    m += (size_t)blk * (size_t)nsrc * BOUND_W;
    double t[NT];
    const double *z[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const int tile = blk * BOUND_W + grp + i * GROUPS;
        t[i] = 0.0;
        z[i] = Z;
        if (tile < tg) {
            const double tv = tau[tile * G + k];
            if (seeds[tile * G + k] >= 0 && tv > 0.0) t[i] = tv;
            z[i] = Z + (size_t)tile * (size_t)n * G + k;
        }
    }
    for (int32_t u = blockIdx.x; u < nsrc; u += gridDim.x) {
        double zv[NT];
#pragma unroll
        for (int i = 0; i < NT; ++i) zv[i] = t[i] > 0.0 ? z[i][(size_t)(src_lo + u) * G] : 0.0;
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            float f = t[i] > 0.0 ? bound_term(zv[i], t[i]) : 0.0f;
#pragma unroll
            for (int sh = G / 2; sh > 0; sh >>= 1) f = fmaxf(f, __shfl_xor(f, sh));
            if (k == 0) m[(size_t)u * BOUND_W + grp + i * GROUPS] = f;
        }
    }
}

// keep bits of the rows[0 .. nrows): lane = tile of the block of BOUND_W tiles, two rows per wave; a lane group fetches up to
// BOUND_W in-link indices with one coalesced load, hands them round (ds_bpermute) and gathers one line of m per in-link, CH
// gathers in flight; the sums run in list order.  A row is kept for a tile unless bound_prunes() says otherwise; a tile flagged
// noprune, a row of more than BOUND_MAX_DEG in-links and a row with a source outside the table are kept untested.
__global__ __launch_bounds__(256) void k_sel_bound_rows(int tg, const int64_t *__restrict__ in_ptr,
                                                        const int32_t *__restrict__ in_src, const int32_t *__restrict__ rows,
                                                        int32_t nrows, int32_t src_lo, int32_t nsrc, const float *__restrict__ m,
                                                        const int32_t *__restrict__ noprune, uint32_t *__restrict__ keep,
                                                        unsigned long long *__restrict__ pruned)
{
    constexpr int RPW = WAVE / BOUND_W, CH = 8;
    const int blk = blockIdx.y;
    const int lane = threadIdx.x & (WAVE - 1);
    const int sub = lane / BOUND_W, k = lane % BOUND_W;
    const int gbase = (lane - k) << 2;
    const int tile = blk * BOUND_W + k;
    const bool real = tile < tg;
    const bool never = real && noprune[tile] != 0;
    m += (size_t)blk * (size_t)nsrc * BOUND_W + k;
    keep += (size_t)blk * (size_t)nrows;
    const int wpb = blockDim.x / WAVE;
    const int64_t nwaves = (int64_t)gridDim.x * wpb;
    unsigned long long skipped = 0;
    for (int64_t rb = ((int64_t)blockIdx.x * wpb + threadIdx.x / WAVE) * RPW; rb < nrows; rb += nwaves * RPW) {
        const int64_t r = rb + sub;
        int64_t p = 0, e = 0;
        if (r < nrows) {
            const int32_t j = rows[r];
            p = in_ptr[j];
            e = in_ptr[j + 1];
        }
        const int64_t deg = e - p;
        if (deg > BOUND_MAX_DEG) e = p;                    // not tested: nothing to sum
        float acc = 0.0f;
        bool outside = false;
        while (__any(p < e)) {
            const int64_t left = e - p;
            const int cnt = left > BOUND_W ? BOUND_W : (left > 0 ? (int)left : 0);
            const int32_t my_idx = (k < cnt) ? in_src[p + k] : src_lo;
            for (int c0 = 0; c0 < BOUND_W; c0 += CH) {
                if (!__any(c0 < cnt)) break;
                float mv[CH];
#pragma unroll
                for (int t = 0; t < CH; ++t) {
                    const int idx = __builtin_amdgcn_ds_bpermute(gbase + ((c0 + t) << 2), my_idx);
                    const uint32_t u = (uint32_t)(idx - src_lo);
                    const bool in = u < (uint32_t)nsrc;
                    mv[t] = (c0 + t < cnt && in) ? m[(size_t)u * BOUND_W] : 0.0f;
                    if (c0 + t < cnt && !in) outside = true;
                }
#pragma unroll
                for (int t = 0; t < CH; ++t) acc += mv[t];
            }
            p += cnt;
        }
        const bool kp = real && (never || outside || !bound_prunes(acc, deg));
        const unsigned long long kb = __ballot(kp), sb = __ballot(real && !kp && r < nrows);
        if (k == 0 && r < nrows) keep[r] = (uint32_t)(kb >> (sub * BOUND_W));
        skipped += (unsigned long long)__popcll(sb);
    }
    if (lane == 0 && skipped) atomicAdd(pruned, skipped);
}

// the tiles' row lists from the keep bits, one pass over the keep words for all tiles of a block of BOUND_W.  A workgroup takes a
// span of COMPACT_SPAN positions; a wave of it COMPACT_RPT runs of 64, so that every load is coalesced and the lanes' positions
// ascend with (wave, run, lane).  Per tile the waves count their kept rows (ballots), one thread per tile reserves the
// workgroup's places with ONE integer atomicAdd and deals them to the waves in order, and the waves write the row ids: inside a
// workgroup's span a list keeps the rows' order in tail_rows[0] (in-degree-descending, which balances k_spmm_select's waves);
// the order of the spans differs from run to run, the rows of a list do not.
constexpr int COMPACT_RPT = 8, COMPACT_WAVES = 4, COMPACT_SPAN = COMPACT_WAVES * WAVE * COMPACT_RPT;
__global__ __launch_bounds__(COMPACT_WAVES * WAVE) void k_sel_bound_compact(int tg, const int32_t *__restrict__ rows, int32_t nrows,
                                                                            const uint32_t *__restrict__ keep,
                                                                            int32_t *__restrict__ list, int32_t *__restrict__ list_cnt)
{
    static_assert(BOUND_W <= WAVE, "one lane per tile of the block");
    __shared__ int32_t wcnt[COMPACT_WAVES][BOUND_W];   // kept rows per (wave, tile), then the wave's first place in the list
    const int blk = blockIdx.y;
    const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
    const uint32_t *kw = keep + (size_t)blk * (size_t)nrows;
    const int64_t nspans = ((int64_t)nrows + COMPACT_SPAN - 1) / COMPACT_SPAN;
    for (int64_t sp = blockIdx.x; sp < nspans; sp += gridDim.x) {
        const int64_t q0 = sp * COMPACT_SPAN + (int64_t)wv * (WAVE * COMPACT_RPT) + lane;
        uint32_t w[COMPACT_RPT];
        int32_t id[COMPACT_RPT];
#pragma unroll
        for (int i = 0; i < COMPACT_RPT; ++i) {
            const int64_t q = q0 + (int64_t)i * WAVE;
            w[i] = q < nrows ? kw[q] : 0u;
            id[i] = q < nrows ? rows[q] : 0;
        }
        int32_t mine = 0;   // lane t < BOUND_W: the wave's kept rows of tile t of the block
        for (int t = 0; t < BOUND_W; ++t) {
            int32_t c = 0;
#pragma unroll
            for (int i = 0; i < COMPACT_RPT; ++i) c += (int32_t)__popcll(__ballot((w[i] >> t) & 1u));
            if (lane == t) mine = c;
        }
        if (lane < BOUND_W) wcnt[wv][lane] = mine;
        __syncthreads();
        if (threadIdx.x < BOUND_W) {
            const int tile = blk * BOUND_W + (int)threadIdx.x;
            int32_t c[COMPACT_WAVES], total = 0;
#pragma unroll
            for (int v = 0; v < COMPACT_WAVES; ++v) total += c[v] = wcnt[v][threadIdx.x];
            int32_t at = (total && tile < tg) ? atomicAdd(&list_cnt[tile], total) : 0;   // (a tile past tg keeps no row)
#pragma unroll
            for (int v = 0; v < COMPACT_WAVES; ++v) { wcnt[v][threadIdx.x] = at; at += c[v]; }
        }
        __syncthreads();
        for (int t = 0; t < BOUND_W; ++t) {
            const int tile = blk * BOUND_W + t;
            if (tile >= tg) break;
            int32_t *out = list + (size_t)tile * (size_t)nrows;
            int32_t at = wcnt[wv][t];
#pragma unroll
            for (int i = 0; i < COMPACT_RPT; ++i) {
                const bool kp = (w[i] >> t) & 1u;
                const unsigned long long bal = __ballot(kp);
                if (kp) out[at + __popcll(bal & ((1ull << lane) - 1ull))] = id[i];
                at += (int32_t)__popcll(bal);
            }
        }
        __syncthreads();   // (wcnt is read until here)
    }
}

// The tiles' row lists (sink->list) of the `count` rows of tail_rows[0] from `first` on (Z: the z matrix the step gathers); *pruned
// (device) receives the (row, tile) pairs skipped.  sink->list stays null with RWR_RANK_PRUNE=0 or without room for the workspace
static int32_t rank_bound_prepare(rwr_graph *g, int G, int tg, const int32_t *d_seeds, const double *Z, int32_t first,
                                  int32_t count, SelSink *sink, unsigned long long **pruned, hipStream_t s)
{
    *pruned = nullptr;
    if (!rank_knobs().prune || !Z || count <= 0 || tg <= 0) return RWR_OK;
    const int32_t *rows = g->tail_rows[0].p + first;
    const size_t nblk = cdiv((size_t)tg, (size_t)BOUND_W);
    const size_t head_bytes = 256 + (((size_t)tg * 2 * sizeof(int32_t) + 255) & ~(size_t)255);   // counter, range | flags, list lengths
    const size_t keep_bytes = (nblk * (size_t)count * sizeof(uint32_t) + 255) & ~(size_t)255;
    auto give_up = [&]() { (void)hipGetLastError(); return RWR_OK; };   // (no room: the unpruned body of before)
    if (g->bound_first != first) {
        // the source rows the body's in-links name: [0, users) on a bipartite like-graph -- the table covers that range only
        if (g->bound_ws.ensure(head_bytes + keep_bytes) != RWR_OK) return give_up();
        int32_t *range = (int32_t *)(g->bound_ws.p + 8);
        const int32_t init[2] = {INT32_MAX, -1};
        int32_t got[2] = {0, 0};
        RWR_HIP(hipMemcpyAsync(range, init, sizeof init, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_sel_bound_range, dim3((unsigned)(cdiv((size_t)count, 256) < 4096 ? cdiv((size_t)count, 256) : 4096)),
                           dim3(256), 0, s, g->in_ptr.p, g->in_src.p, rows, count, range);
        RWR_HIP(hipMemcpyAsync(got, range, sizeof got, hipMemcpyDeviceToHost, s));
        RWR_HIP(hipStreamSynchronize(s));
        g->bound_lo = got[1] >= 0 ? got[0] : 0;
        g->bound_hi = got[1] >= 0 ? got[1] + 1 : 0;
        g->bound_first = first;
    }
    const int32_t nsrc = g->bound_hi - g->bound_lo;
    if (nsrc <= 0) return RWR_OK;   // no in-links at all beyond the head
    const size_t table_bytes = nblk * (size_t)nsrc * BOUND_W * sizeof(float);
    if (g->bound_ws.ensure(head_bytes + keep_bytes + table_bytes) != RWR_OK) return give_up();
    unsigned long long *d_pruned = (unsigned long long *)g->bound_ws.p;
    int32_t *noprune = (int32_t *)(g->bound_ws.p + 256);
    uint32_t *keep = (uint32_t *)(g->bound_ws.p + head_bytes);
    float *m = (float *)(g->bound_ws.p + head_bytes + keep_bytes);
    RWR_HIP(hipMemsetAsync(d_pruned, 0, sizeof(unsigned long long), s));
    hipLaunchKernelGGL(k_sel_bound_flags, dim3(cdiv((size_t)tg, 64)), dim3(64), 0, s, tg, G, d_seeds, sink->tau, noprune);
    const unsigned gt = (unsigned)(cdiv((size_t)nsrc, 4) < 65536 ? cdiv((size_t)nsrc, 4) : 65536);
    RWR_DISPATCH_G(G, {
        if constexpr (GG >= 8)
            hipLaunchKernelGGL(k_sel_bound_table<GG>, dim3(gt, (unsigned)nblk), dim3(256), 0, s, g->n, tg, g->bound_lo, nsrc, Z,
                               d_seeds, sink->tau, m);
    });
    const unsigned want = cdiv((size_t)count, (size_t)(WAVE / BOUND_W) * 4 * 4);
    hipLaunchKernelGGL(k_sel_bound_rows, dim3(want < 1u ? 1u : want < 16384u ? want : 16384u, (unsigned)nblk), dim3(256), 0, s, tg,
                       g->in_ptr.p, g->in_src.p, rows, count, g->bound_lo, nsrc, m, noprune, keep, d_pruned);
    RWR_HIP(hipGetLastError());
    // (the lists live in the frontier lists' buffer, which a batch's first steps are done with and the next call fills anew)
    if (g->fl_rows.ensure((size_t)tg * (size_t)count) != RWR_OK) return give_up();
    int32_t *list_cnt = noprune + tg;
    RWR_HIP(hipMemsetAsync(list_cnt, 0, (size_t)tg * sizeof(int32_t), s));
    const size_t wc = cdiv((size_t)count, (size_t)COMPACT_SPAN);
    hipLaunchKernelGGL(k_sel_bound_compact, dim3((unsigned)(wc < 65536 ? wc : 65536), (unsigned)nblk), dim3(COMPACT_WAVES * WAVE), 0,
                       s, tg, rows, count, keep, g->fl_rows.p, list_cnt);
    RWR_HIP(hipGetLastError());
    sink->list = g->fl_rows.p, sink->list_cnt = list_cnt, sink->list_stride = count;
    *pruned = d_pruned;
    return RWR_OK;
}

// rank.h.  The head (in-degree-descending: tail_rows[0] is a stable partition of row_order) is ranked exactly; its top_n-th
// score bounds the final one from below, and the rest of the step selects by it while it computes
int32_t rank_group_fused(rwr_graph *g, int G, int tg, const int32_t *d_slot_k, const int32_t *d_seeds, int32_t top_n, double *Xf,
                         SplitLast &split, Profile &prof, hipStream_t s, bool *ranked)
{
    const int32_t n_tail = g->tail_n[0];
    const int32_t H = split.head < n_tail ? split.head : n_tail;
    RWR_TRY(rank_group_select(g, G, tg, d_slot_k, top_n, Xf, d_seeds, s, g->tail_rows[0].p, H));
    *ranked = true;
    if (H < n_tail) {
        SelSink sink;
        RWR_TRY(rank_fused_prepare(g, G, tg, d_slot_k, top_n, &sink, s));
        // value-free path: the thresholds bound every body row's scores from one float per in-link, and the
        // selecting launch walks only the rows some seed of the tile may still need (rank_bound.h)
        unsigned long long *d_pruned = nullptr, pruned = 0;
        hipEvent_t b0; RWR_TRY(prof.record(b0, s));
        RWR_TRY(rank_bound_prepare(g, G, tg, d_seeds, split.gi->Zn, H, n_tail - H, &sink, &d_pruned, s));
        RWR_TRY(prof.end(prof.bound, b0, s));
        RWR_TRY(split.gi->redo_rows(split.last, prof, H, n_tail - H, &sink));
        RWR_TRY(rank_fused_merge(g, G, tg, d_slot_k, d_seeds, top_n, sink, s));
        int32_t overflow = 0;   // (one small synchronising copy per group)
        RWR_HIP(hipMemcpyAsync(&overflow, sink.overflow, sizeof(int32_t), hipMemcpyDeviceToHost, s));
        if (d_pruned) RWR_HIP(hipMemcpyAsync(&pruned, d_pruned, sizeof pruned, hipMemcpyDeviceToHost, s));
        RWR_HIP(hipStreamSynchronize(s));
        if (!overflow) g->stats.rank_pruned_rows += (int64_t)pruned;
        if (overflow) {
            // some seed's candidates did not fit: the step again, whole (its inputs are intact), ranked as without the split
            RWR_TRY(split.gi->redo_rows(split.last, prof, 0, -1, nullptr));
            launch_exclude(g, G, tg, Xf, d_seeds, s);
            RWR_HIP(hipGetLastError());
            g->stats.rank_fused_fallbacks += 1;
            *ranked = false;
        }
    }
    g->stats.rank_fused_groups += *ranked;
    return RWR_OK;
}

}  // namespace rwr
