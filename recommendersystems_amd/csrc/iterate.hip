// RWR power iteration  x <- (1-c) P^T x + c e   (Model.deliverRanks / updateRanks,
// Model.cs:76-108) for a batch of seeds, on gfx950.
//
// Data layout: the rank matrix is kept seed-minor, tile by tile:  X[tile][node][G]
// (G = seeds per tile = lanes per row, a power of two <= 64).  One lane owns one
// (destination row, seed) pair and walks the row's in-neighbour list sequentially, so
//   * every in-neighbour access of a lane group is one contiguous G*8-byte row of X
//     (a full 128-byte line at G = 16): coalesced, no per-element gathers;
//   * the addends arrive in exactly the reference's order (source asc, list position
//     asc), so every row except the seed's own is BITWISE what the C# computes -- no
//     reductions, no atomics (SURVEY.md section 3.3 point 1);
//   * pull form writes every y[j] exactly once: updateRanks (Model.cs:103-108) is a
//     pointer swap.
// The seed's own row receives, besides its in-links, the restart mass of EVERY node
// interleaved in node order (Model.cs:91-93,96-97): an n-term sequential fp64 chain per
// seed, reproduced literally by the folds of seed_chain.hip, on a second stream beside the SpMM, or by the parallel binade
// scan of chain_scan.hip (seed_row.h declares both; the SpMM here skips the seeds' own rows).
//
// Arithmetic per edge is the reference's:  rw = (1-d)*x_i  (Model.cs:84), then
// nextRank += rw * weight (Model.cs:87) -- two roundings, never an FMA (the file is built
// with -ffp-contract=off).
//
// This file holds the SpMM half of ONE batched step -- the k_spmm* family, the frontier, mask, seed-initialisation and z
// kernels, their launchers (iterate.h) -- and the host side that carries out a StepPlan (GroupIter, iterate_group), the seed
// row's launches included: their stream choreography is the step's.  Nothing else.  The benchmark's traffic profile
// (profiles/traffic_*.json) carries a fingerprint of this file because the dominant kernels, k_spmm*, live here: they must
// stay here, and neither the seed row's kernels (seed_chain.hip, chain_scan.hip) nor whatever drives the steps for an entry
// point belongs here -- the batched Recommendation is in recommend.hip, Model.run / deliverRanks and the batch of Models in
// model.hip, the row-partitioned mode in partition.hip, the exclusion and ranking in rank.hip.
#include "iterate.h"
#include "bool_dispatch.h"
#include "spmm_chunk.h"

#include <cstdlib>

namespace rwr {

// VF = value-free form (engine.h: rwr_graph::vf): X is then the z matrix -- z[i] = ((1-d) x[i]) * w_src[i], the one
// product Model.cs:87 adds for EVERY link of source i -- no per-entry value is read, a row's sum is the plain list-order
// sum of the gathered z, and the epilogue forms the row's own z for the next step (Zout, may be null on the last one).
template <int G, bool VF>
__global__ __launch_bounds__(256) void k_spmm(int32_t n, const int64_t *__restrict__ in_ptr,
                                              const int32_t *__restrict__ in_src,
                                              const double *__restrict__ in_w,
                                              const int32_t *__restrict__ row_order, int32_t nrows,
                                              const double *__restrict__ X, double *__restrict__ Y,
                                              const int32_t *__restrict__ seeds, double c1, int skip_seed_row,
                                              const double *__restrict__ w_src, double *__restrict__ Zout)
{
    constexpr int RPW = WAVE / G;   // destination rows per wave
    constexpr int U = 4;            // gathers in flight per lane
    const int tile = blockIdx.y;
    const size_t toff = (size_t)tile * (size_t)n * G;
    X += toff;
    Y += toff;
    if (VF && Zout) Zout += toff;
    const int lane = threadIdx.x & (WAVE - 1);
    const int sub = lane / G, k = lane % G;
    const int32_t my_seed = skip_seed_row ? seeds[tile * G + k] : -1;
    const int wpb = blockDim.x / WAVE;
    const int64_t nwaves = (int64_t)gridDim.x * wpb;
    for (int64_t rb = ((int64_t)blockIdx.x * wpb + threadIdx.x / WAVE) * RPW; rb < nrows; rb += nwaves * RPW) {
        const int64_t r = rb + sub;
        int32_t j = -1;
        int64_t p = 0, e = 0;
        if (r < nrows) {
            j = row_order[r];
            p = in_ptr[j];
            e = in_ptr[j + 1];
        }
        double acc = 0.0;
        for (; p + U <= e; p += U) {
            int32_t idx[U];
            double wv[U], xv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) idx[u] = in_src[p + u];
#pragma unroll
            for (int u = 0; u < U; ++u) wv[u] = VF ? 0.0 : in_w[p + u];
#pragma unroll
            for (int u = 0; u < U; ++u) xv[u] = X[(size_t)idx[u] * G + k];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (VF) {
                    acc += xv[u];                // z of the source: the product of Model.cs:84,87, formed once per node
                } else {
                    double rw = c1 * xv[u];      // Model.cs:84
                    acc += rw * wv[u];           // Model.cs:87
                }
            }
        }
        for (; p < e; ++p) {
            if (VF) {
                acc += X[(size_t)in_src[p] * G + k];
            } else {
                double rw = c1 * X[(size_t)in_src[p] * G + k];
                acc += rw * in_w[p];
            }
        }
        if (j >= 0 && j != my_seed) {
            Y[(size_t)j * G + k] = acc;
            if (VF && Zout) { const double rw = c1 * acc; Zout[(size_t)j * G + k] = rw * w_src[j]; }
        }
    }
}

// Chunked variant for G >= 8: a lane group fetches G consecutive in-neighbour indices (and
// weights) of its row with ONE coalesced load -- lane k takes entry p+k -- and hands entry t
// to the whole group through the LDS crossbar (ds_bpermute), instead of G lanes loading the
// same address per edge.  All G row gathers of a chunk are issued before the first add, so
// each lane keeps up to G 8-byte gathers in flight; the adds then run in list order.
// For G > 16 the load is wider than the gather depth: LW = min(G, 32) lanes load -- at 32 one whole 128-byte line of
// in_src, cut by spmm_chunk.h so that each line is fetched once -- and the entries go out in LW / CH rounds of CH gathers.
//
// Frontier awareness for the first iterations (x starts as a single non-zero row per seed and stays
// sparse for two or three steps): CHECK consults a per-tile bitmap "row of X has a non-zero" before a
// row gather and skips the gather of all-zero rows -- their addends are (1-d)*0*w = +0.0, which leave
// the non-negative accumulator bitwise unchanged.  WRITE records the non-zero rows of Y for the next step.
// VF: the value-free form (see k_spmm): X is the z matrix, one index load + one bpermute + one gather + ONE add per
// entry, no weight stream, no multiplies; the epilogue writes the row's next z.
// LIST: the launch walks a row list rather than every row -- the same code; a separate instantiation only so
// that kernel traces and counter passes tell these launches from the dense ones
// SEL: the selecting form of a ranking-only batch's last step (k_spmm_select): no Y, no z -- a lane of a real
// slot whose sum reaches the slot's threshold appends (row, sum) to the slot's candidate buffer (one integer atomicAdd)
// LIVE: a CHECK form whose liveness comes from the step's per-link tile masks (k_entry_live) -- the lane that
// loads in_src[p + k] loads ent_live[p + k] beside it, on the same lines, and tests its tile's bit, instead of probing the
// tile's bitmap at a scattered address.  The bit is the one the probe would have read; everything after it is the same code
template <int G, int CH, bool CHECK, bool WRITE, bool VF, bool SEL = false, bool LIVE = false>
__device__ __forceinline__ void spmm_chunked_body(int32_t n, const int64_t *__restrict__ in_ptr,
                                                  const int32_t *__restrict__ in_src,
                                                  const double *__restrict__ in_w,
                                                  const int32_t *__restrict__ row_order, int32_t nrows,
                                                  const double *__restrict__ X, double *__restrict__ Y,
                                                  const int32_t *__restrict__ seeds, double c1,
                                                  int skip_seed_row, const uint32_t *__restrict__ nz_in,
                                                  uint32_t *__restrict__ nz_out,
                                                  const uint32_t *__restrict__ act,
                                                  const double *__restrict__ w_src, double *__restrict__ Zout,
                                                  const SelSink sink = SelSink{},
                                                  const uint32_t *__restrict__ ent_live = nullptr)
{
    static_assert(G >= 8 && G <= 64, "chunked SpMM needs 8 <= G <= 64");
    static_assert(!SEL || (!CHECK && !WRITE), "the selecting form probes and writes no bitmap");
    static_assert(!LIVE || CHECK, "the per-link masks replace the bitmap probe");
    constexpr int RPW = WAVE / G;
    // entries per index load; CH = entries per gather round.  The weighted forms at G = 64 keep the 16-entry load: with two
    // written-out rounds their probing forms need 98 and 102 instead of 96 and 100 SGPRs, one wave per SIMD fewer.
    constexpr int LW = G <= 32 ? G : VF ? 32 : CH;
    static_assert(LW % CH == 0 && CH <= LW, "an index load is a whole number of gather rounds");
    const int tile = blockIdx.y;
    const size_t toff = (size_t)tile * (size_t)n * G;
    X += toff;
    if (!SEL) Y += toff;
    if (VF && Zout) Zout += toff;
    const size_t nzw = ((size_t)n + 31) / 32;
    if (CHECK && !LIVE) nz_in += (size_t)tile * nzw;
    if (WRITE) nz_out += (size_t)tile * nzw;
    if (CHECK && act) act += (size_t)tile * nzw;
    const int lane = threadIdx.x & (WAVE - 1);
    const int sub = lane / G, k = lane % G;
    const int gbase = (lane - k) << 2;      // byte address of the group's lane 0 for ds_bpermute
    const int32_t my_seed = skip_seed_row ? seeds[tile * G + k] : -1;
    bool sel_real = false;
    double sel_tau = 0.0;
    if (SEL) {
        sel_real = seeds[tile * G + k] >= 0;
        sel_tau = sink.tau[tile * G + k];
    }
    const int wpb = blockDim.x / WAVE;
    const int64_t nwaves = (int64_t)gridDim.x * wpb;
    for (int64_t rb = ((int64_t)blockIdx.x * wpb + threadIdx.x / WAVE) * RPW; rb < nrows; rb += nwaves * RPW) {
        const int64_t r = rb + sub;
        int32_t j = -1;
        int64_t p = 0, e = 0;
        if (r < nrows) {
            j = row_order[r];
            p = in_ptr[j];
            e = in_ptr[j + 1];
            // first iterations: a row none of whose in-neighbours is non-zero (k_mark_active) stays exactly 0
            if (CHECK && act && !((act[(uint32_t)j >> 5] >> (j & 31)) & 1u)) e = p;
        }
        double acc = 0.0;
        // the wave iterates while ANY group still has entries; finished groups idle (cnt = 0)
        while (__any(p < e)) {
            // one load of up to LW entries (spmm_chunk.h: a long list's loads start on 128-byte lines of in_src), then its
            // gather rounds of CH entries each
            const int cnt = spmm_next_load(p, e - p, LW);
            int32_t my_idx = 0;
            double my_w = 0.0;
            if (k < cnt) {
                my_idx = in_src[p + k];
                if (!VF) my_w = in_w[p + k];
                if (LIVE) {    // the link's tile mask, beside its index; dead rows get the sign bit
                    if (!((ent_live[p + k] >> (tile & 31)) & 1u)) my_idx |= (int32_t)0x80000000;
                } else if (CHECK) {   // one bitmap probe per entry (by the lane that fetched it); dead rows get the sign bit
                    const uint32_t wd = nz_in[(uint32_t)my_idx >> 5];
                    if (!((wd >> (my_idx & 31)) & 1u)) my_idx |= (int32_t)0x80000000;
                }
            }
            const int wlo = __double2loint(my_w), whi = __double2hiint(my_w);
            unsigned long long um = 0;
            if (CHECK) {
                // `um` is the union over the wave's row groups of the load's positions that are live in SOME group
                um = __ballot(k < cnt && my_idx >= 0);
                if (G < 64) {
#pragma unroll
                    for (int sh = G; sh < 64; sh <<= 1) um |= um >> sh;
                    um &= (1ull << (G & 63)) - 1ull;
                }
            }
            // the gather rounds of the load.  Rolled where lane groups share a wave: written out, the G = 32 kernels need 80
            // instead of 56 registers.  Written out at G = 64: one group per wave, so every hand-out lane is then a constant
            // (v_readlane, no LDS crossbar), as with 16-entry loads.
#pragma unroll G == 64 ? LW / CH : 1
            for (int r0 = 0; r0 < LW; r0 += CH) {
                if (r0 > 0 && !__any(cnt > r0)) break;   // no group's load reaches this round
                if (CHECK) {
                    // sparse frontier: entries whose source row is all-zero add +0.0 -- skip them wholesale
                    unsigned long long rm = (um >> r0) & ((1ull << CH) - 1ull);
                    if (__popcll(rm) <= 4) {
                        while (rm) {                                  // few live entries: take them one by one, in order
                            const int t = r0 + __builtin_ctzll(rm);
                            rm &= rm - 1;
                            const int idx = __builtin_amdgcn_ds_bpermute(gbase + (t << 2), my_idx);
                            if (VF) {
                                if (t < cnt && idx >= 0) acc += X[(size_t)idx * G + k];
                            } else {
                                const int lo = __builtin_amdgcn_ds_bpermute(gbase + (t << 2), wlo);
                                const int hi = __builtin_amdgcn_ds_bpermute(gbase + (t << 2), whi);
                                if (t < cnt && idx >= 0) {
                                    const double rw = c1 * X[(size_t)idx * G + k];   // Model.cs:84
                                    acc += rw * __hiloint2double(hi, lo);             // Model.cs:87
                                }
                            }
                        }
                        continue;
                    }
                }
                double xv[CH], wv[CH];
#pragma unroll
                for (int t = 0; t < CH; ++t) {
                    const int idx = __builtin_amdgcn_ds_bpermute(gbase + ((r0 + t) << 2), my_idx);
                    if (!VF) {
                        const int lo = __builtin_amdgcn_ds_bpermute(gbase + ((r0 + t) << 2), wlo);
                        const int hi = __builtin_amdgcn_ds_bpermute(gbase + ((r0 + t) << 2), whi);
                        wv[t] = __hiloint2double(hi, lo);
                    }
                    xv[t] = (r0 + t < cnt && idx >= 0) ? X[(size_t)idx * G + k] : 0.0;
                }
#pragma unroll
                for (int t = 0; t < CH; ++t) {
                    if (r0 + t < cnt) {
                        if (VF) {
                            acc += xv[t];                // the source's z: fl(fl((1-d) x) * w), Model.cs:84,87
                        } else {
                            double rw = c1 * xv[t];      // Model.cs:84
                            acc += rw * wv[t];           // Model.cs:87
                        }
                    }
                }
            }
            p += cnt;
        }
        if constexpr (SEL) {
            if (j >= 0 && j != my_seed && sel_real && acc >= sel_tau) {   // (ties at tau are kept)
                const int slot = tile * G + k;
                const int32_t at = atomicAdd(&sink.cursor[slot], 1);
                if (at < sink.cap) sink.cand[(size_t)slot * (size_t)sink.stride + (size_t)at] = RowScore{j, 0, acc};
                else *sink.overflow = 1;
            }
        } else if (j >= 0 && j != my_seed) {
            Y[(size_t)j * G + k] = acc;
            if (VF && Zout) { const double rw = c1 * acc; Zout[(size_t)j * G + k] = rw * w_src[j]; }
        }
        if (WRITE) {
            const unsigned long long nzb = __ballot(acc != 0.0);
            const unsigned long long gmask = (G == 64) ? ~0ull : (((1ull << (G & 63)) - 1ull) << (sub * G));
            if (k == 0 && j >= 0 && (nzb & gmask)) atomicOr(&nz_out[(uint32_t)j >> 5], 1u << (j & 31));
        }
    }
}

template <int G, int CH, bool CHECK, bool WRITE, bool VF, bool LIST>
__global__ __launch_bounds__(256) void k_spmm_chunked(int32_t n, const int64_t *__restrict__ in_ptr,
                                                      const int32_t *__restrict__ in_src,
                                                      const double *__restrict__ in_w,
                                                      const int32_t *__restrict__ row_order, int32_t nrows,
                                                      const double *__restrict__ X, double *__restrict__ Y,
                                                      const int32_t *__restrict__ seeds, double c1,
                                                      int skip_seed_row, const uint32_t *__restrict__ nz_in,
                                                      uint32_t *__restrict__ nz_out,
                                                      const uint32_t *__restrict__ act,
                                                      const double *__restrict__ w_src, double *__restrict__ Zout)
{
    spmm_chunked_body<G, CH, CHECK, WRITE, VF>(n, in_ptr, in_src, in_w, row_order, nrows, X, Y, seeds, c1, skip_seed_row,
                                               nz_in, nz_out, act, w_src, Zout);
}

// The selecting part of a ranking-only batch's last step: the same body over the rest of tail_rows[0], which
// writes no rank: the rows whose sum reaches the slot's threshold tau go to the slot's candidate buffer (SelSink)
template <int G, int CH, bool VF>
__global__ __launch_bounds__(256) void k_spmm_select(int32_t n, const int64_t *__restrict__ in_ptr,
                                                     const int32_t *__restrict__ in_src,
                                                     const double *__restrict__ in_w,
                                                     const int32_t *__restrict__ rows, int32_t nrows,
                                                     const double *__restrict__ X, const int32_t *__restrict__ seeds,
                                                     double c1, const SelSink sink)
{
    // pruned body (rank_bound_prepare): the tile walks its own list of the rows it may still need; its length lives on the device
    if (sink.list) {
        rows = sink.list + (size_t)blockIdx.y * (size_t)sink.list_stride;
        nrows = sink.list_cnt[blockIdx.y];
    }
    spmm_chunked_body<G, CH, false, false, VF, true>(n, in_ptr, in_src, in_w, rows, nrows, X, nullptr, seeds, c1, 1, nullptr,
                                                     nullptr, nullptr, nullptr, nullptr, sink);
}

// Frontier-list steps: the same body over a per-tile row list built by k_mark_active -- tile t walks the
// fl_cnt[t] rows of fl_rows[t * n ...], and no other row of Y / Zout is written.  Every listed row is written whole (all G
// lanes but the seed's own, which the seed-row chain writes).  The count lives on the device: the host never waits for it.
template <int G, int CH, bool VF>
__global__ __launch_bounds__(256) void k_spmm_frontier(int32_t n, const int64_t *__restrict__ in_ptr,
                                                       const int32_t *__restrict__ in_src,
                                                       const double *__restrict__ in_w,
                                                       const int32_t *__restrict__ fl_rows,
                                                       const int32_t *__restrict__ fl_cnt,
                                                       const double *__restrict__ X, double *__restrict__ Y,
                                                       const int32_t *__restrict__ seeds, double c1,
                                                       int skip_seed_row, const uint32_t *__restrict__ nz_in,
                                                       uint32_t *__restrict__ nz_out,
                                                       const double *__restrict__ w_src, double *__restrict__ Zout)
{
    const int tile = blockIdx.y;
    spmm_chunked_body<G, CH, true, true, VF>(n, in_ptr, in_src, in_w, fl_rows + (size_t)tile * (size_t)n, fl_cnt[tile], X, Y,
                                             seeds, c1, skip_seed_row, nz_in, nz_out, nullptr, w_src, Zout);
}

// Per-link tile masks for a probing step that walks every row.  "Is source s live in tile t" is one bit per
// (tile, node) in the frontier bitmaps, which the SpMM would probe once per entry AND tile at a scattered address.  Instead,
// once per step: k_nz_transpose turns the group's bitmaps node-major -- nzT[slab][node], bit t & 31 = node is live in tile
// 32 * slab + (t & 31), tiles past the group's last read as 0 --, and k_entry_live gathers that word once per link, in link
// order: live[slab][e] = nzT[slab][in_src[e]].  A tile's SpMM then reads its slab of `live` beside `in_src`.
// One thread per node and slab: the 32 lanes of a bitmap word read the same word of each tile (one request per wave and tile)
__global__ __launch_bounds__(256) void k_nz_transpose(int32_t n, int tg, const uint32_t *__restrict__ nz, uint32_t *__restrict__ nzT)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t nzw = ((size_t)n + 31) / 32;
    const int slab = blockIdx.y;
    uint32_t out = 0;
#pragma unroll 8
    for (int t = 0; t < 32; ++t) {
        const int tile = slab * 32 + t;
        if (tile < tg) out |= ((nz[(size_t)tile * nzw + (size_t)(i >> 5)] >> (i & 31)) & 1u) << t;
    }
    nzT[(size_t)slab * (size_t)n + (size_t)i] = out;
}
// in_src and live stream; one 4-byte gather per link and slab from the 4 n-byte table of the slab
__global__ __launch_bounds__(256) void k_entry_live(int64_t nnz, int32_t n, int slabs, const int32_t *__restrict__ in_src,
                                                    const uint32_t *__restrict__ nzT, uint32_t *__restrict__ live)
{
    constexpr int U = 4;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e0 < nnz; e0 += U * stride) {
        int32_t src[U];
#pragma unroll
        for (int u = 0; u < U; ++u) src[u] = e0 + u * stride < nnz ? in_src[e0 + u * stride] : -1;
        for (int sl = 0; sl < slabs; ++sl) {
            uint32_t v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = src[u] >= 0 ? nzT[(size_t)sl * (size_t)n + (size_t)src[u]] : 0u;
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (src[u] >= 0) live[(size_t)sl * (size_t)nnz + (size_t)(e0 + u * stride)] = v[u];
        }
    }
}
// ... and the probing SpMM over every row that reads them: the k_spmm_chunked body with its liveness from the tile's slab
template <int G, int CH, bool WRITE, bool VF>
__global__ __launch_bounds__(256) void k_spmm_entry_live(int32_t n, const int64_t *__restrict__ in_ptr,
                                                         const int32_t *__restrict__ in_src,
                                                         const double *__restrict__ in_w,
                                                         const int32_t *__restrict__ row_order, int32_t nrows,
                                                         const double *__restrict__ X, double *__restrict__ Y,
                                                         const int32_t *__restrict__ seeds, double c1,
                                                         int skip_seed_row, uint32_t *__restrict__ nz_out,
                                                         const uint32_t *__restrict__ act,
                                                         const double *__restrict__ w_src, double *__restrict__ Zout,
                                                         const uint32_t *__restrict__ live, int64_t nnz)
{
    spmm_chunked_body<G, CH, true, WRITE, VF, false, true>(n, in_ptr, in_src, in_w, row_order, nrows, X, Y, seeds, c1,
                                                           skip_seed_row, nullptr, nz_out, act, w_src, Zout, SelSink{},
                                                           live + (size_t)(blockIdx.y >> 5) * (size_t)nnz);
}

// First iterations: destination rows that can become non-zero = out-neighbours (explicit links) of the rows of X
// that hold a non-zero.  One thread per bitmap word of the tile; pushes over the RAW out-links.
// fl_rows != nullptr (frontier-list step): also the tile's row list -- the lane whose atomicOr sets a new
// bit appends the row (one atomicAdd per wave), and the tile's seed rows are marked and listed too, so that every row the
// step writes is written whole.  Each row enters a tile's list once.
__global__ __launch_bounds__(256) void k_mark_active(int32_t n, const uint32_t *__restrict__ nz, uint32_t *__restrict__ act,
                                                     const int64_t *__restrict__ rowptr, const int32_t *__restrict__ dst,
                                                     const uint8_t *__restrict__ etype, int G, const int32_t *__restrict__ seeds,
                                                     int32_t *__restrict__ fl_rows, int32_t *__restrict__ fl_cnt)
{
    // one WAVE per bitmap word; the lanes stride over the out-links of each non-zero row of that word
    const size_t nzw = ((size_t)n + 31) / 32;
    const int tile = blockIdx.y;
    const int lane = threadIdx.x & (WAVE - 1);
    const size_t wi = (size_t)blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE;
    uint32_t *a = act + (size_t)tile * nzw;
    int32_t *list = fl_rows ? fl_rows + (size_t)tile * (size_t)n : nullptr;
    if (list && blockIdx.x == 0 && threadIdx.x < (unsigned)G) {
        const int32_t sr = seeds[tile * G + threadIdx.x];
        if (sr >= 0) {
            const uint32_t bit = 1u << (sr & 31);
            if (!(atomicOr(&a[(uint32_t)sr >> 5], bit) & bit)) list[atomicAdd(&fl_cnt[tile], 1)] = sr;
        }
    }
    if (wi >= nzw) return;
    uint32_t w = nz[(size_t)tile * nzw + wi];
    while (w) {
        const int b = __builtin_ctz(w);
        w &= w - 1;
        const int64_t i = (int64_t)wi * 32 + b;
        const int64_t p1 = rowptr[i + 1];
        if (!list) {
            for (int64_t p = rowptr[i] + lane; p < p1; p += WAVE)
                if (etype[p] != RWR_EDGE_UNDEFINED) {
                    const int32_t t = dst[p];
                    atomicOr(&a[(uint32_t)t >> 5], 1u << (t & 31));
                }
            continue;
        }
        for (int64_t p0 = rowptr[i]; p0 < p1; p0 += WAVE) {   // (i is wave-uniform: every lane takes the same trips)
            const int64_t p = p0 + lane;
            bool add = false;
            int32_t t = 0;
            if (p < p1 && etype[p] != RWR_EDGE_UNDEFINED) {
                t = dst[p];
                const uint32_t bit = 1u << (t & 31);
                add = !(atomicOr(&a[(uint32_t)t >> 5], bit) & bit);
            }
            const unsigned long long m = __ballot(add);
            if (!m) continue;
            const int leader = __builtin_ctzll(m);
            int base = 0;
            if (lane == leader) base = atomicAdd(&fl_cnt[tile], (int)__popcll(m));
            base = __shfl(base, leader);
            const int below = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            if (add) list[base + below] = t;
        }
    }
}

// Model ctor, Model.cs:42-49: rank[seed] = nNodes, everything else 0
// (value-free path: Z receives the seed's z, ((1-d) n) * w_src[seed])
// Each seed row is written whole -- n in the lanes whose seed it is, 0 in the others -- so that it is valid even where the
// matrix was not cleared (Z on the frontier-list path).  Slots that share a seed row write the same values.
__global__ void k_init_seeds(int32_t n, int ntiles, int G, double *__restrict__ X,
                             const int32_t *__restrict__ seeds, uint32_t *__restrict__ nz,
                             double *__restrict__ Z = nullptr, const double *__restrict__ w_src = nullptr, double c1 = 0.0)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= ntiles * G) return;
    const int32_t s = seeds[q];
    if (s < 0) return;
    const int tile = q / G;
    const size_t row = (size_t)tile * (size_t)n * G + (size_t)s * G;
    const double rw = c1 * (double)n;
    const double zs = Z ? rw * w_src[s] : 0.0;
    for (int kk = 0; kk < G; ++kk) {
        const bool mine = seeds[tile * G + kk] == s;
        X[row + kk] = mine ? (double)n : 0.0;
        if (Z) Z[row + kk] = mine ? zs : 0.0;
    }
    if (nz) atomicOr(&nz[(size_t)tile * (((size_t)n + 31) / 32) + ((uint32_t)s >> 5)], 1u << (s & 31));
}

// value-free path: the z of the seeds' own rows, once the seed-row kernel (chain / scan / restart reduction) has
// left their final rank in Y:  z = ((1-d) * y) * w_src   (the product of Model.cs:84,87 for the next step)
__global__ void k_seed_z(int32_t n, int ntiles, int G, const double *__restrict__ Y, double *__restrict__ Z,
                         const int32_t *__restrict__ seeds, const double *__restrict__ w_src, double c1)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= ntiles * G) return;
    const int32_t s = seeds[q];
    if (s < 0) return;
    const size_t at = (size_t)(q / G) * (size_t)n * G + (size_t)s * G + (q % G);
    const double rw = c1 * Y[at];
    Z[at] = rw * w_src[s];
}
// value-free path, rank vector supplied by the caller (Model.deliverRanks on its own): z of every row
__global__ __launch_bounds__(256) void k_make_z(int64_t elems, int G, const double *__restrict__ X, double *__restrict__ Z,
                                                const double *__restrict__ w_src, double c1)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= elems) return;
    const double rw = c1 * X[q];
    Z[q] = rw * w_src[q / G];
}

// row-partitioned mode, first steps: z of the slab's rows AND the bitmap of the rows that hold a non-zero (global row numbers).
// A thread per row, counted from the 64-aligned row at or below the slab's first: a wave then covers exactly two words of the
// bitmap and writes them whole (no atomics; the words of rows outside the slab stay as the memset left them).
__global__ __launch_bounds__(256) void k_make_z_nz(int32_t lo, int32_t hi, int G, const double *__restrict__ X, double *__restrict__ Zs,
                                                   const double *__restrict__ w_src, double c1, uint32_t *__restrict__ nz)
{
    const int64_t j = ((int64_t)lo & ~(int64_t)63) + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;     // global row
    bool any = false;
    if (j >= lo && j < hi) {
        const double w = w_src[j];
        const size_t at = (size_t)(j - lo) * G;
        for (int k = 0; k < G; ++k) {
            const double xv = X[(size_t)j * G + k];
            const double rw = c1 * xv;
            Zs[at + k] = rw * w;
            any = any || xv != 0.0;
        }
    }
    const unsigned long long m = __ballot(any);
    const int lane = threadIdx.x & (WAVE - 1);
    if (lane == 0 && (uint32_t)m) nz[(uint64_t)j >> 5] = (uint32_t)m;
    if (lane == 32 && (uint32_t)(m >> 32)) nz[(uint64_t)j >> 5] = (uint32_t)(m >> 32);
}

// ------------------------------------------------------------------------------ host side

// The plan's environment values, read once per process (the RWR_TUNE_ENV ones only by the experiments build)
static PlanInput read_plan_knobs()
{
    PlanInput v;
    const char *e;
    if ((e = getenv("RWR_SPMM"))) v.spmm = atoi(e);
    if ((e = RWR_TUNE_ENV("RWR_NZ_ITERS"))) v.nz_iters = atoi(e);
    if ((e = getenv("RWR_ACT_ITERS"))) v.act_iters = atoi(e);
    if ((e = RWR_TUNE_ENV("RWR_ACT_MIN_N"))) v.act_min_n = atol(e);
    if ((e = getenv("RWR_FRONTIER_LIST"))) v.frontier_list = atoi(e);
    if ((e = getenv("RWR_CHAIN"))) v.chain = atoi(e);
    if ((e = RWR_TUNE_ENV("RWR_SCAN_WORK"))) v.scan_work = atof(e);
    if ((e = RWR_TUNE_ENV("RWR_SCAN_SIDE"))) v.scan_side = atoi(e);
    if ((e = RWR_TUNE_ENV("RWR_GATE"))) v.gate = atoi(e);
    if ((e = getenv("RWR_TAIL_ROWS"))) v.tail_rows = atoi(e);
    if ((e = RWR_TUNE_ENV("RWR_CHAIN_SERIAL"))) v.two_streams = atoi(e) == 0;
    if ((e = getenv("RWR_X_CLEAR"))) v.x_clear = atoi(e);
    if ((e = getenv("RWR_ENTRY_LIVE"))) v.entry_live = atoi(e);
    return v;
}
static const PlanInput &plan_knobs() { static const PlanInput k = read_plan_knobs(); return k; }
// the most a group's per-link tile masks may take (RWR_ENTRY_LIVE_CAP_MB, default 4 GB: C4's one slab takes 0.8 GB, C3's six
// 1.2 GB); a group past it keeps the bitmap probe
static size_t entry_live_cap_bytes()
{
    static const size_t v = [] {
        const char *e = getenv("RWR_ENTRY_LIVE_CAP_MB");
        const long long mb = e ? atoll(e) : 4096;
        return (size_t)(mb > 0 ? mb : 0) << 20;
    }();
    return v;
}

// (frontier lists, DESIGN §3.3.2: their lengths only the device knows; the grid is sized for a list of a tenth of the rows --
// the lists of C4's frontier steps hold 0.05 % and 4 % -- and the launch strides over longer ones)
template <int G>
static void launch_spmm_g(rwr_graph *g, int tg, const SpmmArgs &a, hipStream_t s)
{
    const bool vf = a.Zin != nullptr;
    const double *GS = vf ? a.Zin : a.X;   // gather source
    const int skip = a.skip_seed_row;
    constexpr int RPW = WAVE / G;
    constexpr int CH = G > 16 ? 16 : G;   // entries per chunk = row gathers in flight per lane
    if constexpr (G >= 8) {
        if (a.rows.kind == Rows::Frontier) {
            const int32_t *fl_rows = g->fl_rows.p, *fl_cnt = g->fl_rows.p + (size_t)tg * (size_t)g->n;
            const unsigned want = cdiv((size_t)g->n / 10 + 1, (size_t)RPW * 4);
            const unsigned gx = want < 1u ? 1u : want < 2048u ? want : 2048u;
            bool_dispatch([&](auto v) {
                hipLaunchKernelGGL((k_spmm_frontier<G, CH, decltype(v)::value>), dim3(gx, tg), dim3(256), 0, s, g->n, g->in_ptr.p,
                                   g->in_src.p, g->in_w.p, fl_rows, fl_cnt, GS, a.Y, a.seeds, a.c1, skip, a.nz_in, a.nz_out,
                                   g->w_src.p, a.Zout);
            }, vf);
            return;
        }
    }
    const bool listed = a.rows.kind == Rows::Tail;
    const int32_t *order = listed ? g->tail_rows[a.rows.level].p : g->row_order.p;
    int32_t nrows = listed ? g->tail_n[a.rows.level] : g->n;
    if (listed) {   // a part of the level's list
        const int32_t first = a.row_first < nrows ? a.row_first : nrows;
        order += first;
        nrows = (a.row_count >= 0 && a.row_count < nrows - first) ? a.row_count : nrows - first;
    }
    if (nrows <= 0 && (a.sel || a.row_count >= 0)) return;   // an empty part
    unsigned want = cdiv((size_t)nrows, (size_t)RPW * 4);
    unsigned gx = want < 1u ? 1u : want < 8192u ? want : 8192u;
    if constexpr (G == 1) {
        if (tg == 1 && plan_knobs().spmm != 0) {   // (every row: the callers pass no row list to this path)
            launch_spmv_exact(g, a.X, a.Y, a.seeds, a.c1, skip, a.act, a.nz_out, s, a.Zin, a.Zout, a.hub_scan);
            return;
        }
    }
    if constexpr (G >= 8) {
        if (a.sel) {   // (split_last_ok: only with the chunked kernels)
            const SelSink sink = *a.sel;
            bool_dispatch([&](auto v) {
                hipLaunchKernelGGL((k_spmm_select<G, CH, decltype(v)::value>), dim3(gx, tg), dim3(256), 0, s, g->n, g->in_ptr.p,
                                   g->in_src.p, g->in_w.p, order, nrows, GS, a.seeds, a.c1, sink);
            }, vf);
            return;
        }
    }
    if constexpr (G >= 8) {
        if (a.ent_live && a.nz_in && !listed && plan_knobs().spmm != 0) {   // a probing step over every row, masks built
            bool_dispatch([&](auto wr, auto v) {
                hipLaunchKernelGGL((k_spmm_entry_live<G, CH, decltype(wr)::value, decltype(v)::value>), dim3(gx, tg), dim3(256), 0,
                                   s, g->n, g->in_ptr.p, g->in_src.p, g->in_w.p, order, nrows, GS, a.Y, a.seeds, a.c1, skip,
                                   a.nz_out, a.act, g->w_src.p, a.Zout, a.ent_live, g->nnz);
            }, a.nz_out != nullptr, vf);
            return;
        }
    }
    if constexpr (G >= 8) {
        if (plan_knobs().spmm != 0) {
            bool_dispatch([&](auto chk, auto wr, auto v, auto lst) {
                if constexpr (decltype(chk)::value || !decltype(wr)::value)
                    hipLaunchKernelGGL((k_spmm_chunked<G, CH, decltype(chk)::value, decltype(wr)::value, decltype(v)::value,
                                                       decltype(lst)::value>), dim3(gx, tg), dim3(256), 0, s, g->n, g->in_ptr.p,
                                       g->in_src.p, g->in_w.p, order, nrows, GS, a.Y, a.seeds, a.c1, skip, a.nz_in, a.nz_out,
                                       a.act, g->w_src.p, a.Zout);
            }, a.nz_in != nullptr, a.nz_in && a.nz_out, vf, listed);
            return;
        }
    }
    bool_dispatch([&](auto v) {
        hipLaunchKernelGGL((k_spmm<G, decltype(v)::value>), dim3(gx, tg), dim3(256), 0, s, g->n, g->in_ptr.p, g->in_src.p,
                           g->in_w.p, order, nrows, GS, a.Y, a.seeds, a.c1, skip, g->w_src.p, a.Zout);
    }, vf);
}
void launch_spmm(rwr_graph *g, int G, int tg, const SpmmArgs &a, hipStream_t s)
{
    RWR_DISPATCH_G(G, launch_spmm_g<GG>(g, tg, a, s));
}
void launch_init_seeds(rwr_graph *g, int G, int tg, double *X, const int32_t *seeds, uint32_t *nz, double *Z, double c1,
                       hipStream_t s)
{
    hipLaunchKernelGGL(k_init_seeds, dim3(cdiv((size_t)tg * G, 64)), dim3(64), 0, s, g->n, tg, G, X, seeds, nz, Z, g->w_src.p, c1);
}
void launch_make_z(int64_t elems, int G, const double *X, double *Z, const double *w_src, double c1, hipStream_t s)
{
    hipLaunchKernelGGL(k_make_z, dim3(cdiv((size_t)elems, 256)), dim3(256), 0, s, elems, G, X, Z, w_src, c1);
}
void launch_make_z_nz(rwr_graph *g, int32_t lo, int32_t hi, int G, const double *X, double *Zs, double c1, uint32_t *nz,
                      hipStream_t s)
{
    const int64_t first = (int64_t)lo & ~(int64_t)63;
    hipLaunchKernelGGL(k_make_z_nz, dim3(cdiv((size_t)((int64_t)hi - first), 256)), dim3(256), 0, s, lo, hi, G, X, Zs, g->w_src.p,
                       c1, nz);
}
void launch_mark_active(rwr_graph *g, int G, int tg, const uint32_t *nz, uint32_t *act, const int32_t *seeds, int32_t *fl_rows,
                        int32_t *fl_cnt, hipStream_t s)
{
    const size_t nzw = ((size_t)g->n + 31) / 32;
    hipLaunchKernelGGL(k_mark_active, dim3(cdiv(nzw, 4), tg), dim3(256), 0, s, g->n, nz, act, g->rowptr.p, g->dst.p, g->etype.p,
                       G, seeds, fl_rows, fl_cnt);
}

int32_t Profile::record(hipEvent_t &e, hipStream_t s)
{
    e = nullptr;
    if (!on) return RWR_OK;
    if (used == pool.size()) { RWR_HIP(hipEventCreate(&e)); pool.push_back(e); }
    e = pool[used++];
    RWR_HIP(hipEventRecord(e, s));
    return RWR_OK;
}
int32_t Profile::end(std::vector<hipEvent_t> &stage, hipEvent_t a, hipStream_t s)
{
    hipEvent_t b; RWR_TRY(record(b, s));
    if (on) stage.insert(stage.end(), {a, b});
    return RWR_OK;
}
int32_t Profile::fold(rwr_graph *g)
{
    auto drain = [&](const std::vector<hipEvent_t> &v, double *acc, bool dense_only) -> int32_t {
        for (size_t i = 0; i + 1 < v.size(); i += 2) {
            float ms = 0.f;
            if (dense_only && !dense[i / 2]) continue;
            RWR_HIP(hipEventElapsedTime(&ms, v[i], v[i + 1]));
            *acc += ms;
        }
        return RWR_OK;
    };
    if (on) {
        RWR_TRY(drain(spmm, &g->stats.spmm_dense_ms, true));
        RWR_TRY(drain(spmm, &g->stats.spmm_ms, false));
        RWR_TRY(drain(chain, &g->stats.chain_ms, false));
        RWR_TRY(drain(rank, &g->stats.rank_ms, false));
        RWR_TRY(drain(iter, &g->stats.iterate_wall_ms, false));
        RWR_TRY(drain(bound, &g->stats.rank_bound_ms, false));
    }
    reset();
    return RWR_OK;
}

int32_t GroupIter::init(bool fresh, bool ranks_nonneg, bool ranking_only)
{
    const int32_t n = g->n;
    hipStream_t s = g->stream;
    const size_t elems = (size_t)tg * (size_t)n * G;
    PlanInput in = plan_knobs();
    in.n = n; in.nnz = g->nnz; in.nonneg = g->nonneg; in.big_n = spmv_big_n(); in.seed_row_kernel = g->opts.seed_row_kernel;
    in.scan_self = chain_scan_self_contained(G); in.G = G; in.tg = tg; in.c1 = c1;
    in.fresh = fresh; in.ranks_nonneg = ranks_nonneg; in.ranking_only = ranking_only;
    cfg = plan_config(in);
    if (!fresh && Zc) launch_make_z((int64_t)elems, G, X, Zc, g->w_src.p, c1, s);
    const size_t nzw = ((size_t)n + 31) / 32;
    if (cfg.flist && g->fl_rows.ensure((size_t)tg * (size_t)n + (size_t)tg) != RWR_OK) {
        (void)hipGetLastError();   // (no room for the lists: the bitmap-probing steps of before, which need none)
        cfg.flist = false;
        cfg.clear_x = plan_clear_x(cfg);
    }
    if (cfg.entry_live) {   // the group's per-link tile masks: one word per link and 32 tiles, and the node-major bitmaps
        const size_t slabs = ((size_t)tg + 31) / 32, words = slabs * (size_t)g->nnz;
        if (g->nnz <= 0 || words > entry_live_cap_bytes() / sizeof(uint32_t) || g->ent_nzT.ensure(slabs * (size_t)n) != RWR_OK ||
            g->ent_live.ensure(words) != RWR_OK) {
            (void)hipGetLastError();   // (past the cap, or no room: the per-entry bitmap probe of before, which needs neither)
            cfg.entry_live = false;
        }
    }
    // X_0 is zero outside the seed rows.  On the frontier-list path every reader of steps 0 to 2 goes through the frontier
    // bitmaps, so the seed rows (k_init_seeds) are all of X that must be valid: no clear
    if (fresh && cfg.clear_x) RWR_HIP(hipMemsetAsync(X, 0, elems * sizeof(double), s));
    if (fresh && !cfg.clear_x) g->stats.x_clear_skipped += 1;
    // Z is read only through the frontier bitmaps until a step has written it whole: on the frontier-list path the
    // seed rows (k_init_seeds) are all of it that must be valid
    if (fresh && Zc && !cfg.flist) RWR_HIP(hipMemsetAsync(Zc, 0, elems * sizeof(double), s));
    nz_cur = cfg.nz_iters > 0 ? g->d_nz.p : nullptr;
    nz_oth = cfg.nz_iters > 0 ? g->d_nz.p + (size_t)tg * nzw : nullptr;
    if (nz_cur) RWR_HIP(hipMemsetAsync(nz_cur, 0, (size_t)tg * nzw * sizeof(uint32_t), s));
    if (fresh) launch_init_seeds(g, G, tg, X, d_seeds, nz_cur, Zc, c1, s);
    RWR_HIP(hipGetLastError());
    if (cfg.scan) RWR_TRY(chain_scan_prepare(g, G, tg, d_seeds, s));
    if (Zc && G == 1 && tg == 1 && cfg.addends_nonneg) RWR_TRY(sweep_prepare(g));   // single seed: the source-block sweep (sweep.hip)
    // (the simple one-lane reference kernel of the seed row walks the weighted in-lists itself)
    if (Zc && cfg.chain_kind == 0 && !cfg.scan) RWR_TRY(ensure_in_w(g));
    return RWR_OK;
}

int32_t GroupIter::step(const StepPlan &p, Profile &prof, int32_t row_first, int32_t row_count)
{
    const int32_t n = g->n;
    hipStream_t s = g->stream;
    const size_t nzw = ((size_t)n + 31) / 32;
    constexpr int GATE_SLOTS = 64;
    const uint32_t *nz_in = p.probe ? nz_cur : nullptr;
    uint32_t *nz_out = p.write_bits ? nz_oth : nullptr;
    if (nz_out) RWR_HIP(hipMemsetAsync(nz_out, 0, (size_t)tg * nzw * sizeof(uint32_t), s));
    uint32_t *act = p.mark ? g->d_nz.p + 2 * (size_t)tg * nzw : nullptr;
    const bool listed = p.rows.kind == Rows::Frontier;
    if (act) {
        int32_t *fl_rows = listed ? g->fl_rows.p : nullptr, *fl_cnt = listed ? fl_rows + (size_t)tg * (size_t)n : nullptr;
        RWR_HIP(hipMemsetAsync(act, 0, (size_t)tg * nzw * sizeof(uint32_t), s));
        if (fl_cnt) RWR_HIP(hipMemsetAsync(fl_cnt, 0, (size_t)tg * sizeof(int32_t), s));
        launch_mark_active(g, G, tg, nz_in, act, d_seeds, fl_rows, fl_cnt, s);
    }
    // Per-link tile masks of this step's frontier, on the main stream.  Every writer of nz_cur is behind this
    // point of it: init's memset and k_init_seeds, or the step before -- its memset, its SpMM (WRITE) and its chain, whose
    // second stream that step joined (ev_join) before it returned.  Nothing in this step writes nz_cur
    const uint32_t *ent_live = nullptr;
    if (p.entry_live && nz_in) {
        const int slabs = (tg + 31) / 32;
        hipLaunchKernelGGL(k_nz_transpose, dim3(cdiv((size_t)n, 256), slabs), dim3(256), 0, s, n, tg, nz_in, g->ent_nzT.p);
        const unsigned want = cdiv((size_t)g->nnz, 256 * 4);
        hipLaunchKernelGGL(k_entry_live, dim3(want < 1u ? 1u : want < (1u << 20) ? want : (1u << 20)), dim3(256), 0, s, g->nnz, n,
                           slabs, g->in_src.p, g->ent_nzT.p, g->ent_live.p);
        ent_live = g->ent_live.p;
        g->stats.entry_live_launches += 1;
    }
    const uint32_t *nz_terms = p.terms_nz ? nz_in : nullptr;
    double *zout = (Zc && p.form_z) ? Zn : nullptr;
    hipStream_t sc = p.chain_side ? g->stream2 : s;   // the chain's stream
    unsigned int *gate_it = p.gate ? g->d_gate.p + (it % GATE_SLOTS) : nullptr;
    if (p.chain != Chain::None) {
        // A fold: its link terms on the main stream ahead of the fork (launch_seed_terms), then the fold beside the SpMM.
        // The binade scan: on the main stream ahead of the SpMM (which skips the seed rows), or for a single seed on the
        // second stream beside the SpMV -- the two read the same vectors and write disjoint rows.
        if (!p.scan()) launch_seed_terms(g, G, tg, X, d_seeds, c1, d_evoff, s, Zc, nz_terms);
        if (gate_it) RWR_HIP(hipMemsetAsync(gate_it, 0, sizeof(unsigned int), s));
        if (p.chain_side) { RWR_HIP(hipEventRecord(g->ev_fork, s)); RWR_HIP(hipStreamWaitEvent(sc, g->ev_fork, 0)); }
        if (p.scan() && !(p.chain_self && Zc)) launch_seed_terms(g, G, tg, X, d_seeds, c1, d_evoff, sc, Zc, nz_terms);
        hipEvent_t c0; RWR_TRY(prof.record(c0, sc));
        if (p.scan())
            RWR_TRY(chain_scan_step(g, G, tg, X, Y, d_seeds, d_evoff, c1, nz_out, sc, p.chain_self ? Zc : nullptr,
                                    p.chain_self ? zout : nullptr));
        else
            launch_chain(g, G, tg, X, Y, d_seeds, c1, d_evoff, nz_out, gate_it, sc, p.chain, nz_in, p.chain_masked);
        RWR_TRY(prof.end(prof.chain, c0, sc));
        if (p.chain_side) RWR_HIP(hipEventRecord(g->ev_join, sc));
    }
    if (gate_it) launch_gate(gate_it, (unsigned)(tg < 192 ? tg : 192), s);
    hipEvent_t a; RWR_TRY(prof.record(a, s));
    SpmmArgs sp;
    sp.X = X, sp.Y = Y, sp.seeds = d_seeds, sp.c1 = c1, sp.skip_seed_row = true;
    sp.nz_in = nz_in, sp.nz_out = nz_out, sp.act = act, sp.Zin = Zc, sp.Zout = zout;
    sp.hub_scan = cfg.addends_nonneg, sp.rows = p.rows;
    sp.row_first = row_first, sp.row_count = row_count;
    sp.ent_live = ent_live;
    launch_spmm(g, G, tg, sp, s);
    RWR_TRY(prof.end(prof.spmm, a, s));
    if (prof.on) prof.dense.push_back(p.dense());
    if (p.dense()) { g->stats.spmm_dense_launches += 1; ++dense_steps; }
    if (p.chain_side) RWR_HIP(hipStreamWaitEvent(s, g->ev_join, 0));
    // value-free path: the seed rows' own z, now that the seed-row kernel has left their rank in Y
    if (zout && p.seed_z) hipLaunchKernelGGL(k_seed_z, dim3(cdiv((size_t)tg * G, 64)), dim3(64), 0, s, n, tg, G, Y, zout, d_seeds, g->w_src.p, c1);
    RWR_HIP(hipGetLastError());
    { double *t = X; X = Y; Y = t; }   // Model.updateRanks (Model.cs:103-108)
    { double *t = Zc; Zc = Zn; Zn = t; }
    { uint32_t *tz = nz_cur; nz_cur = nz_oth; nz_oth = tz; }
    g->stats.spmm_launches += 1;
    g->stats.chain_launches += p.chain != Chain::None; g->stats.frontier_list_launches += listed;
    ++it;
    return RWR_OK;
}

int32_t GroupIter::redo_rows(const StepPlan &p, Profile &prof, int32_t row_first, int32_t row_count, const SelSink *sel)
{
    // step() has swapped the buffers: Y holds the ranks the step read and Zn their z; X is what it wrote
    hipStream_t s = g->stream;
    hipEvent_t a; RWR_TRY(prof.record(a, s));
    SpmmArgs sp;
    sp.X = Y, sp.Y = X, sp.seeds = d_seeds, sp.c1 = c1, sp.skip_seed_row = true;
    sp.Zin = Zn, sp.Zout = nullptr;
    sp.hub_scan = cfg.addends_nonneg, sp.rows = p.rows;
    sp.row_first = row_first, sp.row_count = row_count, sp.sel = sel;
    launch_spmm(g, G, tg, sp, s);
    RWR_TRY(prof.end(prof.spmm, a, s));
    if (prof.on) prof.dense.push_back(0);
    RWR_HIP(hipGetLastError());
    return RWR_OK;
}

// A tile group of the batched Recommendation: T steps of the plan (iterate.h)
int32_t iterate_group(rwr_graph *g, int G, int tg, const int32_t *d_seeds, const int64_t *d_evoff, const int32_t *h_seeds,
                      double d, int64_t T, Profile &prof, double **final_X, int64_t *dense_steps, SplitLast *split)
{
    GroupIter gi(g, G, tg, d_seeds, d_evoff, d);
    // (a batch of no steps ranks X_0 itself: every row must be valid, so it takes the plan of a caller that reads the ranks)
    RWR_TRY(gi.init(true, true, /*ranking_only=*/T >= 1));
    if (gi.cfg.tails) {
        RWR_TRY(tail_rows_prepare(g));
        gi.cfg.tail_depth = g->tail_depth;
        for (size_t q = 0; q < (size_t)tg * G; ++q)
            if (h_seeds[q] >= 0) gi.cfg.need |= g->h_tail_flag[h_seeds[q]];
    }
    // the last step in two parts: a chainless, probe-free walk of tail level 0 by the chunked kernels only
    bool split_ok = false;
    if (split && split->head > 0 && T >= 1 && G >= 8 && plan_knobs().spmm != 0) {
        const StepPlan last = plan_step(gi.cfg, T - 1, T);
        split_ok = last.rows.kind == Rows::Tail && last.rows.level == 0 && !last.probe && !last.write_bits && !last.form_z &&
                   last.chain == Chain::None;
        split->last = last;
    }
    while (gi.it < T) {
        const StepPlan p = plan_step(gi.cfg, gi.it, T);
        if (split_ok && gi.it == T - 1) RWR_TRY(gi.step(p, prof, 0, split->head));
        else RWR_TRY(gi.step(p, prof));
    }
    if (split_ok) { split->taken = true; split->gi.emplace(gi); }
    *final_X = gi.X;
    *dense_steps = gi.dense_steps;
    return RWR_OK;
}

}  // namespace rwr
