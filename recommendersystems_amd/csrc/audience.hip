// The audience of an item (rwr_recommend_audience_batch): given K targets, rank for each the seeds whose
// personalised walk of T steps would score it highest -- without walking from any seed.
//
// The forward score x_T^(s)[v] of target v, for every seed s at once, is a polynomial in the transition matrix applied to
// e_v from the other side: with the reverse step  B(g)[i] = (1-d) * sum_{e in raw list of i} w_e * g[dst_e]  (w_e = the
// normalised weight, 0 for an UNDEFINED link, so a dangling row gives 0),
//     g_0 = e_v,  g_{j+1} = B(g_j),   S[s] = sum_{j < T} rho_{T-1-j}[s] * g_j[s]  +  n * g_T[s],
// where rho_k[s] = d n + (1-d) delta_k[s] is the restart mass of seed s's walk at step k and delta_k[s] the mass that walk holds
// on dangling nodes.  delta comes from the same step applied to the dangling indicator (h_0 = dangling, h_{j+1} = B(h_j)) and a
// recurrence per node (audience_plan.h: aud_rho_node); on a graph without dangling nodes rho is the constant d n.
//
// K targets fill the columns of the [tile][n][G] matrices the forward batch uses: two g buffers and the accumulator S, which
// the ranked end (ranked_end.h) then takes as its X -- candidate rows of a type, -1 marks, top-N select, copy-back.  The marks
// of the audience look at IN-links: k_audience_exclude walks the raw lists once and marks the sources of the masked links
// into a target.
//
// Arithmetic: every addend is >= 0; a row's addends are summed in list order, each as one fma; no floating-point atomics.  A
// column's values depend on its target, d, T and the graph alone -- not on its lane, its tile, G or the batch.  The result
// is NOT bitwise the forward walk's (the addends arrive in another order): rwr.h states the derived tolerance.
//
// Weighted target sets (rwr_recommend_audience_set_batch and its positions entry): the walk is linear in its
// start and rho does not depend on the target, so set k = {(v, a_v)} is the same T steps from g_0 = sum_v a_v e_v
// (k_rev_init_sets, from audience_set_plan.h's merged pairs).  The one body runs an AudCall: sets, pool, deny lists and the
// list or positions destination; rwr_recommend_audience_batch fills it with one-member unit sets.
#include "audience.h"

#include "audience_plan.h"
#include "audience_set_plan.h"
#include "explain.h"
#include "filter.h"
#include "iterate.h"
#include "long_list.h"
#include "ranked_end.h"

namespace rwr {

// ---- the reverse step -------------------------------------------------------------------------------------------------------
// The batched SpMM's mapping (iterate.hip: k_spmm): a lane owns one (row, column) pair, the G lanes of a group gather one
// G * 8-byte row of g per link -- a whole 128-byte line at G = 16 -- and every lane adds its column's addends in list order.

// links [p, e) of one raw list over the tile's g: sum of w_e * g[dst_e][k], list order.  A link of weight 0 (UNDEFINED, or an
// explicit link of raw weight 0) adds +0.0 to a sum that is >= +0.0 and is not gathered.  wave_short: no lane group of the
// wave has more than AUD_SHORT links -- the loads, the gathers and the adds are then issued without a loop, predicated.
template <int G>
__device__ __forceinline__ double rev_list_sum(int64_t p, int64_t e, const int32_t *__restrict__ dst, const double *__restrict__ w,
                                               const double *__restrict__ gin, int k, bool wave_short)
{
    constexpr int U = AUD_SHORT;
    double acc = 0.0;
    if (wave_short) {
        int32_t idx[U];
        double wv[U], xv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool on = p + u < e;
            idx[u] = on ? dst[p + u] : 0;
            wv[u] = on ? w[p + u] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) xv[u] = wv[u] != 0.0 ? gin[(size_t)idx[u] * G + k] : 0.0;
#pragma unroll
        for (int u = 0; u < U; ++u) acc = fma(wv[u], xv[u], acc);
        return acc;
    }
    for (; p + U <= e; p += U) {
        int32_t idx[U];
        double wv[U], xv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) idx[u] = dst[p + u];
#pragma unroll
        for (int u = 0; u < U; ++u) wv[u] = w[p + u];
#pragma unroll
        for (int u = 0; u < U; ++u) xv[u] = wv[u] != 0.0 ? gin[(size_t)idx[u] * G + k] : 0.0;
#pragma unroll
        for (int u = 0; u < U; ++u) acc = fma(wv[u], xv[u], acc);
    }
    for (; p < e; ++p) {
        const double wv = w[p];
        if (wv != 0.0) acc = fma(wv, gin[(size_t)dst[p] * G + k], acc);
    }
    return acc;
}

// One reverse step of a tile group: gout = B(gin) over the first AUD_SPLIT links of every row (a longer row leaves its
// unscaled first-piece sum, which k_rev_join finishes), and in the same pass S[i] += rho[i] * gin[i] (S == nullptr: the
// dangling column, which accumulates nothing; rho == nullptr: the constant rho_const).
template <int G>
__global__ __launch_bounds__(256) void k_rev_spmm(int32_t n, const int64_t *__restrict__ rowptr, const int32_t *__restrict__ dst,
                                                  const double *__restrict__ w, const double *__restrict__ gin,
                                                  double *__restrict__ gout, double *__restrict__ S,
                                                  const double *__restrict__ rho, double rho_const, double c1)
{
    constexpr int RPW = WAVE / G;
    const size_t toff = (size_t)blockIdx.y * (size_t)n * G;
    gin += toff;
    gout += toff;
    if (S) S += toff;
    const int lane = threadIdx.x & (WAVE - 1);
    const int sub = lane / G, k = lane % G;
    const int wpb = blockDim.x / WAVE;
    const int64_t nwaves = (int64_t)gridDim.x * wpb;
    for (int64_t rb = ((int64_t)blockIdx.x * wpb + threadIdx.x / WAVE) * RPW; rb < n; rb += nwaves * RPW) {
        const int64_t i = rb + sub;
        int64_t p = 0, e = 0, e_all = 0;
        if (i < n) {
            p = rowptr[i];
            e_all = rowptr[i + 1];
            e = aud_first_piece_end(p, e_all);
        }
        const bool wave_short = !__any(e - p > AUD_SHORT);
        const double acc = rev_list_sum<G>(p, e, dst, w, gin, k, wave_short);
        if (i < n) {
            const size_t at = (size_t)i * G + k;
            gout[at] = e_all > e ? acc : c1 * acc;
            if (S) S[at] = fma(rho ? rho[i] : rho_const, gin[at], S[at]);
        }
    }
}

// ... the further pieces of the rows of more than AUD_SPLIT links (audience_plan.h: aud_long_rows), one lane group per
// piece: part[piece][tile][G] = the piece's list-order sum
template <int G>
__global__ __launch_bounds__(256) void k_rev_pieces(int32_t n, int32_t npieces, const int64_t *__restrict__ piece_p0,
                                                    const int64_t *__restrict__ piece_p1, const int32_t *__restrict__ dst,
                                                    const double *__restrict__ w, const double *__restrict__ gin,
                                                    double *__restrict__ part)
{
    constexpr int RPW = WAVE / G;
    const int tile = blockIdx.y, tg = gridDim.y;
    gin += (size_t)tile * (size_t)n * G;
    const int lane = threadIdx.x & (WAVE - 1);
    const int sub = lane / G, k = lane % G;
    const int wpb = blockDim.x / WAVE;
    const int64_t nwaves = (int64_t)gridDim.x * wpb;
    for (int64_t rb = ((int64_t)blockIdx.x * wpb + threadIdx.x / WAVE) * RPW; rb < npieces; rb += nwaves * RPW) {
        const int64_t q = rb + sub;
        int64_t p = 0, e = 0;
        if (q < npieces) { p = piece_p0[q]; e = piece_p1[q]; }
        const double acc = rev_list_sum<G>(p, e, dst, w, gin, k, false);
        if (q < npieces) part[((size_t)q * tg + tile) * G + k] = acc;
    }
}

// ... and their second pass, in a fixed order: gout[row] = (1-d) * (((first piece + piece 1) + piece 2) + ...).  One thread
// per (long row, tile, column).
__global__ __launch_bounds__(256) void k_rev_join(int32_t n, int G, int tg, int32_t nlong, const int32_t *__restrict__ row,
                                                  const int32_t *__restrict__ first, const double *__restrict__ part,
                                                  double *__restrict__ gout, double c1)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= (int64_t)nlong * tg * G) return;
    const int k = (int)(j % G), tile = (int)((j / G) % tg);
    const int32_t r = (int32_t)(j / ((int64_t)G * tg));
    const size_t at = (size_t)tile * (size_t)n * G + (size_t)row[r] * G + k;
    double acc = gout[at];
    for (int32_t q = first[r]; q < first[r + 1]; ++q) acc += part[((size_t)q * tg + tile) * G + k];
    gout[at] = c1 * acc;
}

// g_0 of a group: the merged weight at (member row, slot's column) of every (slot, member) pair of the group
// (audience_set_plan.h: aud_set_pairs), one thread per pair; the matrix was cleared.  The pairs' cells are distinct after the
// merge, so a store serves and no order matters.  A one-member unit set stores the 1.0 a single target's column starts from.
__global__ __launch_bounds__(256) void k_rev_init_sets(int32_t n, int G, int nslots, int32_t npairs, const int32_t *__restrict__ pair_slot,
                                                       const int32_t *__restrict__ pair_row, const double *__restrict__ pair_w,
                                                       double *__restrict__ g0)
{
    const int32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= npairs) return;
    const int32_t q = pair_slot[j], v = pair_row[j];
    if (q < 0 || q >= nslots || v < 0 || v >= n) return;         // (the plan names slots of the group and rows of [0, n) only)
    g0[(size_t)(q / G) * (size_t)n * G + (size_t)v * G + (q % G)] = pair_w[j];
}

// after the last step: S += n * g_T
__global__ __launch_bounds__(256) void k_rev_final(int64_t elems, double nn, const double *__restrict__ gT, double *__restrict__ S)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < elems; j += stride) S[j] = fma(nn, gT[j], S[j]);
}

// ---- the dangling column and the restart mass ----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_rev_h0(int32_t n, const uint8_t *__restrict__ dangling, double *__restrict__ h0)
{
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) h0[i] = dangling[i] ? 1.0 : 0.0;
}

// rho[k][i] for k < T from h[j][i] for j < T: audience_plan.h's recurrence, one thread per node (neighbouring threads read
// neighbouring cells of every table row)
__global__ __launch_bounds__(256) void k_rev_rho(int32_t n, double d, int32_t T, const double *__restrict__ h, double *__restrict__ rho)
{
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) aud_rho_node(n, d, T, h + i, (size_t)n, rho + i, (size_t)n);
}

// ---- the exclusion: the sources of the masked links INTO a target ------------------------------------------------------------
__global__ __launch_bounds__(256) void k_aud_mark_targets(int32_t n, int32_t cnt, const int32_t *__restrict__ tn, uint32_t *__restrict__ bitmap)
{
    const int32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= cnt) return;
    const int32_t v = tn[j];
    if (v >= 0 && v < n) atomicOr(&bitmap[(uint32_t)v >> 5], 1u << (v & 31));
}

// One pass over the raw lists, a thread per link: a link whose type has its bit in the mask (ranked_end.hip's test: a type
// beyond the mask's width is never masked) and whose target is one of the group's (bitmap, then the sorted table tn[0 .. cnt))
// marks its source row -- found by a search of rowptr, for these few links only -- in every column the target owns
// (tslot[tptr[e] .. tptr[e + 1]): group-local slots).  Two links of one source to one target store the same -1.
__global__ __launch_bounds__(256) void k_audience_exclude(int32_t n, int G, int nslots, int64_t nnz_raw, const int64_t *__restrict__ rowptr,
                                                          const int32_t *__restrict__ dst, const uint8_t *__restrict__ etype,
                                                          uint32_t mask, const uint32_t *__restrict__ bitmap, int32_t cnt,
                                                          const int32_t *__restrict__ tn, const int32_t *__restrict__ tptr,
                                                          const int32_t *__restrict__ tslot, double *__restrict__ X)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < nnz_raw; p += stride) {
        const uint32_t t = etype[p];
        if (t >= TYPED_EDGE_TYPES || !((mask >> t) & 1u)) continue;
        const int32_t v = dst[p];
        if (v < 0 || v >= n || !((bitmap[(uint32_t)v >> 5] >> (v & 31)) & 1u)) continue;
        const int32_t e = aud_target_find(tn, cnt, v);
        if (e < 0) continue;
        const int32_t src = aud_link_row(rowptr, n, p);
        for (int32_t a = tptr[e]; a < tptr[e + 1]; ++a) {
            const int32_t q = tslot[a];
            if (q >= 0 && q < nslots) X[(size_t)(q / G) * (size_t)n * G + (size_t)src * G + (q % G)] = -1.0;
        }
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
namespace {

template <class T>
int32_t upload_vec(DevBuf<T> &d, const std::vector<T> &h, hipStream_t s)
{
    RWR_TRY(d.alloc(h.size()));
    if (!h.empty()) RWR_HIP(hipMemcpyAsync(d.p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, s));
    return RWR_OK;
}

unsigned rev_blocks(int64_t units, int G)
{
    const int64_t per_block = (int64_t)(WAVE / G) * 4;           // 4 waves of WAVE / G lane groups
    int64_t b = (units + per_block - 1) / per_block;
    if (b < 1) b = 1;
    if (b > (1 << 20)) b = 1 << 20;                              // (the kernels stride over what is left)
    return (unsigned)b;
}

// the device copies of the long-row plan and the partial sums of one step
struct LongRows {
    int32_t nlong = 0, npieces = 0;
    DevBuf<int32_t> row, first;
    DevBuf<int64_t> p0, p1;
    DevBuf<double> part;
};

// one whole reverse step of tg tiles of width G on s: the main launch, then the long rows' pieces and their join
int32_t rev_step(rwr_graph *g, int G, int tg, const LongRows &L, const double *gin, double *gout, double *S, const double *rho,
                 double rho_const, double c1, hipStream_t s)
{
    const int32_t n = g->n;
    RWR_DISPATCH_G(G, hipLaunchKernelGGL((k_rev_spmm<GG>), dim3(rev_blocks(n, GG), (unsigned)tg), dim3(256), 0, s, n, g->rowptr.p,
                                         g->dst.p, g->w_norm_raw.p, gin, gout, S, rho, rho_const, c1));
    if (L.npieces > 0) {
        RWR_DISPATCH_G(G, hipLaunchKernelGGL((k_rev_pieces<GG>), dim3(rev_blocks(L.npieces, GG), (unsigned)tg), dim3(256), 0, s, n,
                                             L.npieces, L.p0.p, L.p1.p, g->dst.p, g->w_norm_raw.p, gin, L.part.p));
        const int64_t cells = (int64_t)L.nlong * tg * G;
        hipLaunchKernelGGL(k_rev_join, dim3(cdiv((size_t)cells, 256)), dim3(256), 0, s, n, G, tg, L.nlong, L.row.p, L.first.p,
                           L.part.p, gout, c1);
    }
    RWR_HIP(hipGetLastError());
    return RWR_OK;
}

}  // namespace

int32_t audience_body(rwr_graph *g, const AudCall &call, double d, const char *who)
{
    const double t_begin = now_ms();
    const int32_t n = g->n, T = call.n_iter, K = call.K;
    const double c1 = 1 - d, nn = (double)n;
    const uint32_t etype_mask = call.etype_mask;
    hipStream_t s = g->stream;
    // (the end and what it points to are declared before idle: ranked_end.h's lifetime rule; so is every scratch buffer)
    WhyEnd why;                                                  // no reasons (T = 0, n_why = 0): only the entries' rows
    why.nodes = call.out_node;
    LongEnd lng;                                                 // rwr_recommend_audience_set_long_batch beyond the select's limit
    lng.nodes = call.out_node;
    PosEnd pe;                                                   // (set up as typed.hip sets up the filtered positions entry's)
    pe.ev.test_ptr = call.test_ptr, pe.ev.test_ids = call.test_ids;
    pe.pos_out = call.out_pos, pe.score_out = call.out_score, pe.list_len = call.out_len;
    RankedEnd end;
    end.who = who;
    if (call.dest == AUD_LISTS) {
        end.top_n = call.top_n, end.ids = call.out_id, end.scores = call.out_score, end.counts = call.out_count;
        if (long_applies(call.top_n)) end.lng = &lng;            // (only the long entry's ladder lets such a top_n through)
        else if (call.out_node) end.why = &why;
    } else {
        end.pos = &pe;
    }
    end.deny_ptr = call.deny_ptr, end.deny_idx = call.deny_idx;
    Profile prof(g);
    DevBuf<int32_t> own_rows;
    DevBuf<double> rho, h;
    LongRows L;
    DevBuf<uint32_t> t_bitmap;
    DevBuf<int32_t> t_node, t_ptr, t_slot, p_slot, p_row;
    DevBuf<double> p_w;
    if (call.n_pool >= 0 || call.cand_type == FILTER_ANY_TYPE) {
        RWR_TRY(filter_rows_build(g, call.cand_type, call.n_pool, call.pool_idx, own_rows, &end.nrows, prof));
        end.rows = own_rows.p;
    } else {
        RWR_TRY(cand_rows_get(g, call.cand_type, &end.rows, &end.nrows));
    }

    // the long rows of the current raw lists, and the tables of rho and h, before the workspace is sized from what is free
    const AudLongRows plan = aud_long_rows(n, g->h_rowptr.data());
    if (plan.too_many) { set_error("%s: too many long-row pieces", who); return RWR_E_UNSUPPORTED; }
    bool any_dangling = false;
    for (int32_t i = 0; i < n && !any_dangling; ++i) any_dangling = g->h_dangling[(size_t)i] != 0;
    const uint64_t rho_elems = aud_rho_elems(T, n, any_dangling);
    if (rho_elems > 0) {
        RWR_TRY(rho.alloc((size_t)rho_elems));
        RWR_TRY(h.alloc((size_t)rho_elems));
    }
    const int G = resolve_G(g, K);
    int TG = 1;
    // three [tile][n][G] matrices: S = X, and the two g buffers -- Y and, on a value-free graph, Z0 (which the workspace of
    // such a graph holds anyway), else cs_diff as the one extra matrix
    RWR_TRY(ensure_workspace(g, G, K, &TG, g->vf ? 0 : 1));
    double *S = g->X.p, *ga = g->Y.p, *gb = g->vf ? g->Z0.p : g->cs_diff.p;
    const int ntiles = (int)cdiv((size_t)K, (size_t)G);
    // the sets are dealt to the slots by their first members (a column's values do not depend on its slot)
    std::vector<int32_t> slot_k, first_member((size_t)K);
    for (int32_t k = 0; k < K; ++k) first_member[(size_t)k] = call.set_idx[call.set_ptr[k]];
    RWR_TRY(upload_seed_slots(g, first_member.data(), K, G, &slot_k));
    // the members' own rows: the end's (slot, member) pairs over the caller's sets; the in-links are marked here, so its mask is 0
    end.set_ptr = call.set_ptr, end.set_idx = call.set_idx, end.mask = 0, end.members = call.exclude_members != 0;
    // (a host vector that is uploaded outlives the stream's work, like the device buffers)
    const AudSets merged = aud_set_merge(K, call.set_ptr, call.set_idx, call.set_w);
    const AudSetPairs pairs = aud_set_pairs(merged, slot_k.size(), slot_k.data(), (size_t)TG * G);
    const AudTargets tt = etype_mask != 0 ? aud_set_targets(merged, slot_k.size(), slot_k.data(), (size_t)TG * G) : AudTargets{};
    if (pairs.slot.size() > 0x7FFFFFFFull) { set_error("%s: too many set members", who); return RWR_E_UNSUPPORTED; }
    StreamsIdle idle{g};
    RWR_TRY(end.prepare(g, K, slot_k, (size_t)TG * G, s));

    L.nlong = (int32_t)plan.row.size(), L.npieces = (int32_t)plan.piece_row.size();
    if (L.npieces > 0) {
        RWR_TRY(upload_vec(L.row, plan.row, s));
        RWR_TRY(upload_vec(L.first, plan.first, s));
        RWR_TRY(upload_vec(L.p0, plan.piece_p0, s));
        RWR_TRY(upload_vec(L.p1, plan.piece_p1, s));
        RWR_TRY(L.part.alloc((size_t)aud_part_elems((uint64_t)L.npieces, TG, G)));
    }
    RWR_TRY(upload_vec(p_slot, pairs.slot, s));
    RWR_TRY(upload_vec(p_row, pairs.row, s));
    RWR_TRY(upload_vec(p_w, pairs.w, s));
    if (etype_mask != 0) {
        RWR_TRY(upload_vec(t_node, tt.node, s));
        RWR_TRY(upload_vec(t_ptr, tt.ptr, s));
        RWR_TRY(upload_vec(t_slot, tt.slot, s));
        RWR_TRY(t_bitmap.alloc(((size_t)n + 31) / 32));
    }

    // the restart mass: h_0 = dangling, h_{j+1} = B(h_j) with the K = 1 form of the step, then the recurrence per node
    if (rho_elems > 0) {
        hipEvent_t r0; RWR_TRY(prof.record(r0, s));
        hipLaunchKernelGGL(k_rev_h0, dim3(cdiv((size_t)n, 256)), dim3(256), 0, s, n, g->dangling.p, h.p);
        for (int32_t j = 0; j + 1 < T; ++j)
            RWR_TRY(rev_step(g, 1, 1, L, h.p + (size_t)j * n, h.p + (size_t)(j + 1) * n, nullptr, nullptr, 0.0, c1, s));
        hipLaunchKernelGGL(k_rev_rho, dim3(cdiv((size_t)n, 256)), dim3(256), 0, s, n, d, T, h.p, rho.p);
        RWR_HIP(hipGetLastError());
        RWR_TRY(prof.end(prof.chain, r0, s));
    }

    for (int t0 = 0, grp = 0; t0 < ntiles; t0 += TG, ++grp) {
        const int tg = (ntiles - t0 < TG) ? (ntiles - t0) : TG;
        const size_t q0 = (size_t)t0 * G, elems = (size_t)aud_mat_elems(tg, n, G);
        hipEvent_t i0; RWR_TRY(prof.record(i0, s));
        RWR_HIP(hipMemsetAsync(S, 0, elems * sizeof(double), s));
        RWR_HIP(hipMemsetAsync(ga, 0, elems * sizeof(double), s));
        const int64_t m0 = pairs.group_off[(size_t)grp], npairs = pairs.group_off[(size_t)grp + 1] - m0;
        if (npairs > 0)
            hipLaunchKernelGGL(k_rev_init_sets, dim3(cdiv((size_t)npairs, 256)), dim3(256), 0, s, n, G, tg * G, (int32_t)npairs,
                               p_slot.p + m0, p_row.p + m0, p_w.p + m0, ga);
        double *cur = ga, *nxt = gb;
        for (int32_t j = 0; j < T; ++j) {                        // S += rho_{T-1-j} * g_j, g_{j+1} = B(g_j)
            hipEvent_t a; RWR_TRY(prof.record(a, s));
            RWR_TRY(rev_step(g, G, tg, L, cur, nxt, S, rho_elems > 0 ? rho.p + (size_t)(T - 1 - j) * n : nullptr, d * nn, c1, s));
            RWR_TRY(prof.end(prof.spmm, a, s));
            if (prof.on) prof.dense.push_back(0);
            g->stats.spmm_launches += 1;
            double *sw = cur; cur = nxt; nxt = sw;
        }
        hipLaunchKernelGGL(k_rev_final, dim3(cdiv(elems < ((size_t)1 << 28) ? elems : ((size_t)1 << 28), 256)), dim3(256), 0, s,
                           (int64_t)elems, nn, cur, S);
        RWR_HIP(hipGetLastError());
        RWR_TRY(prof.end(prof.iter, i0, s));
        int32_t real = 0;
        for (size_t q = q0; q < q0 + (size_t)tg * G; ++q) real += slot_k[q] >= 0;
        g->stats.spmm_seed_steps += (int64_t)real * T;

        if (etype_mask != 0) {                                   // booked with the ranked end: rank_ms
            hipEvent_t x0; RWR_TRY(prof.record(x0, s));
            const int64_t e0 = tt.group_off[(size_t)grp];
            const int32_t cnt = (int32_t)(tt.group_off[(size_t)grp + 1] - e0);
            if (cnt > 0 && g->nnz_raw > 0) {
                RWR_HIP(hipMemsetAsync(t_bitmap.p, 0, (((size_t)n + 31) / 32) * sizeof(uint32_t), s));
                hipLaunchKernelGGL(k_aud_mark_targets, dim3(cdiv((size_t)cnt, 256)), dim3(256), 0, s, n, cnt, t_node.p + e0, t_bitmap.p);
                const size_t blocks = cdiv((size_t)g->nnz_raw, 256);
                hipLaunchKernelGGL(k_audience_exclude, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, s, n, G, tg * G,
                                   g->nnz_raw, g->rowptr.p, g->dst.p, g->etype.p, etype_mask, t_bitmap.p, cnt, t_node.p + e0,
                                   t_ptr.p + e0, t_slot.p, S);
                RWR_HIP(hipGetLastError());
            }
            RWR_TRY(prof.end(prof.rank, x0, s));
        }
        RWR_TRY(end.finish_group(g, G, tg, grp, q0, S, prof, s, nullptr));
    }
    RWR_TRY(end.copy_back(g, K));
    g->stats.seeds_done += K;
    return finish_model_batch(g, prof, G, TG, t_begin);
}

}  // namespace rwr
