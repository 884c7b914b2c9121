// At most m candidates per caller-set group of nodes in every seed's ranked list (rwr_recommend_capped_batch,
// rwr_recommend_capped_positions_batch).  The walk, the exclusion, the pool, the deny lists and the
// destinations are the filtered entries' (typed.hip's driver, ranked_end.h); what is this file's is the stage between the deny
// marks and the destination: per group and per column of the rank matrix, the cells outside the best m receive -1.
//
// Per call (cap_build): the labelled rows of the candidate list become sorted keys (label << 32 | row), their segment heads
// are compacted and read back once, and cap_plan.h cuts the segments longer than m into chunks.  Per tile group (cap_group):
// one wave per (chunk, tile) keeps every column's best m keys in registers -- lanes across the G columns, 64 / G rows in
// flight per trip, the sub-lanes' lists merged by cross-lane shuffles.  A one-chunk segment is marked by the same wave in a
// second pass over its rows; a longer one writes its chunks' lists, one wave per (segment, tile) merges them into the
// thresholds, and a launch of its own marks.  Nothing is computed, only compared: the kept cells are untouched, the dropped
// ones hold the -1 of every other exclusion, and the result does not depend on the launches' schedule.
#include "group_cap.h"

#include <cstdlib>

#include "filter.h"

namespace rwr {

static_assert(CAP_MAX == RWR_GROUP_CAP_MAX, "cap_plan.h's list and the header's limit are one number");

// ---- keys and segment heads: count per block, scan of the counts, ordered scatter (typed.hip's k_cand_*, cap_plan.h) ----------

enum { CAP_ITEM_LABELLED = 0, CAP_ITEM_HEAD = 1 };

// does this thread's item match, and the wave's matches as a ballot; wc[w] = matches of wave w of the workgroup.
// LABELLED: item p is position p of the candidate list, it matches when its row carries a label >= 0; HEAD: item p is
// position p of the sorted keys, it matches when a segment begins there
template <int ITEM>
__device__ __forceinline__ bool cap_item_match(int32_t count, int32_t n, const int32_t *__restrict__ rows,
                                               const int32_t *__restrict__ label, const uint64_t *__restrict__ sorted, int32_t *wc,
                                               unsigned long long *bal, uint64_t *key)
{
    const int32_t b = blockIdx.x;
    const int32_t p = cand_block_lo(b) + (int32_t)threadIdx.x;
    bool m = false;
    *key = 0;
    if (p < cand_block_hi(b, count)) {
        if (ITEM == CAP_ITEM_LABELLED) {
            const int32_t r = rows[p];
            if (r >= 0 && r < n) {                                // (the lists hold rows of [0, n) only)
                const int32_t lb = label[r];
                m = lb >= 0;
                *key = cap_key(lb, r);
            }
        } else {
            m = cap_is_head(sorted, p);
            *key = (uint64_t)(uint32_t)p;
        }
    }
    *bal = __ballot(m);
    if ((threadIdx.x & (WAVE - 1)) == 0) wc[threadIdx.x / WAVE] = __popcll(*bal);
    __syncthreads();
    return m;
}

template <int ITEM>
__global__ __launch_bounds__(CAND_BLOCK) void k_cap_count(int32_t count, int32_t n, const int32_t *__restrict__ rows,
                                                          const int32_t *__restrict__ label, const uint64_t *__restrict__ sorted,
                                                          int32_t *__restrict__ block_cnt)
{
    __shared__ int32_t wc[CAND_BLOCK / WAVE];
    unsigned long long bal;
    uint64_t key;
    cap_item_match<ITEM>(count, n, rows, label, sorted, wc, &bal, &key);
    if (threadIdx.x == 0) {
        int32_t c = 0;
        for (int w = 0; w < CAND_BLOCK / WAVE; ++w) c += wc[w];
        block_cnt[blockIdx.x] = c;
    }
}

// LABELLED: keys[pos] = the row's key, vals[pos] = the row; HEAD: start[pos] = the head's position
template <int ITEM>
__global__ __launch_bounds__(CAND_BLOCK) void k_cap_scatter(int32_t count, int32_t n, const int32_t *__restrict__ rows,
                                                            const int32_t *__restrict__ label, const uint64_t *__restrict__ sorted,
                                                            const int32_t *__restrict__ off, int32_t total, uint64_t *__restrict__ keys,
                                                            uint32_t *__restrict__ vals, int32_t *__restrict__ start)
{
    __shared__ int32_t wc[CAND_BLOCK / WAVE];
    unsigned long long bal;
    uint64_t key;
    if (!cap_item_match<ITEM>(count, n, rows, label, sorted, wc, &bal, &key)) return;
    const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
    int32_t pos = off[blockIdx.x];
    for (int q = 0; q < wv; ++q) pos += wc[q];
    pos += __popcll(bal & ((1ull << lane) - 1ull));
    if (pos < 0 || pos >= total) return;
    if (ITEM == CAP_ITEM_LABELLED) {
        keys[pos] = key;
        vals[pos] = (uint32_t)key;
    } else {
        start[pos] = (int32_t)(uint32_t)key;
    }
}

// ---- the selection ------------------------------------------------------------------------------------------------------------

constexpr int CAP_TRIPS = 4;   // trips of 64 / G rows whose loads are issued before the first compare

// The cells of positions [pos, pos + len) of the sorted keys in this lane's column (xt = the tile's X + the column), 64 / G
// rows per trip, sub-lane `sub` at the trip's row `sub`: the live ones go through `f(x, id, row)`.  The rows of a segment are
// scattered over n -- G x 8-byte row gathers, the SpMM's access shape -- so the loads of CAP_TRIPS trips (keys, then cells
// and ids) are all issued before the first cell is looked at.
template <int G, class F>
__device__ __forceinline__ void cap_walk_rows(const uint64_t *__restrict__ sorted, int32_t pos, int32_t len, int32_t n,
                                              const double *xt, const int64_t *__restrict__ node_id, bool live_lane, F &&f)
{
    constexpr int R = WAVE / G;
    const int sub = (int)threadIdx.x / G;
    for (int32_t b = 0; b < len; b += R * CAP_TRIPS) {
        int32_t row[CAP_TRIPS];
        double x[CAP_TRIPS];
        int64_t id[CAP_TRIPS];
#pragma unroll
        for (int u = 0; u < CAP_TRIPS; ++u) {
            const int32_t p = b + u * R + sub;
            row[u] = (p < len && live_lane) ? cap_key_row(sorted[(size_t)pos + p]) : -1;
            if (row[u] >= n) row[u] = -1;                        // (keys are built from rows of [0, n))
        }
#pragma unroll
        for (int u = 0; u < CAP_TRIPS; ++u) {
            x[u] = -1.0, id[u] = 0;
            if (row[u] >= 0) {
                x[u] = xt[(size_t)row[u] * G];
                id[u] = node_id[row[u]];
            }
        }
#pragma unroll
        for (int u = 0; u < CAP_TRIPS; ++u)
            if (x[u] >= 0.0) f(x[u], id[u], row[u]);
    }
}

// the lists of the 64 / G sub-lanes of a column become one, in every sub-lane (a butterfly of shuffles: every lane takes part)
template <int G>
__device__ __forceinline__ void cap_merge_sublanes(CapList &l)
{
#pragma unroll
    for (int o = G; o < WAVE; o <<= 1) {
        CapList other;
#pragma unroll
        for (int j = 0; j < CAP_MAX; ++j) {
            other.k[j].hi = (uint64_t)__shfl_xor((unsigned long long)l.k[j].hi, o);
            other.k[j].lo = (uint64_t)__shfl_xor((unsigned long long)l.k[j].lo, o);
            other.k[j].rw = (uint32_t)__shfl_xor((int)l.k[j].rw, o);
        }
        cap_list_merge(l, other);
    }
}

template <int G>
__device__ __forceinline__ void cap_mark_rows(const CapKey &thr, const uint64_t *__restrict__ sorted, int32_t pos, int32_t len,
                                              int32_t n, double *xt, const int64_t *__restrict__ node_id, bool live_lane)
{
    cap_walk_rows<G>(sorted, pos, len, n, xt, node_id, live_lane, [&](double x, int64_t id, int32_t row) {
        if (cap_better(thr, cap_rank_key(x, id, row))) xt[(size_t)row * G] = -1.0;
    });
}

// One wave per (chunk list[blockIdx.x], tile blockIdx.y).  FUSED (one-chunk segments): select, then mark the same rows --
// the wave touches its own chunk's cells only.  Otherwise the column's m keys go to part[tile][blockIdx.x][i][column].
template <int G, bool FUSED>
__global__ __launch_bounds__(WAVE) void k_cap_select(int32_t n, int32_t m, int32_t nlist, const int32_t *__restrict__ list,
                                                     const int32_t *__restrict__ chunk_pos, const int32_t *__restrict__ chunk_len,
                                                     const uint64_t *__restrict__ sorted, const int64_t *__restrict__ node_id,
                                                     const int32_t *__restrict__ slot_k, double *X, uint64_t *__restrict__ part_hi,
                                                     uint64_t *__restrict__ part_lo, uint32_t *__restrict__ part_rw)
{
    const int32_t j = blockIdx.x, tile = blockIdx.y;
    if (j >= nlist) return;
    const int32_t c = list[j];
    const int32_t pos = chunk_pos[c], len = chunk_len[c];
    const int col = (int)threadIdx.x % G;
    const bool live_lane = slot_k[(size_t)tile * G + col] >= 0;   // (a padding slot's column holds nothing to rank)
    double *xt = X + (size_t)tile * (size_t)n * G + col;
    CapList l;
    cap_list_init(l, m);
    cap_walk_rows<G>(sorted, pos, len, n, xt, node_id, live_lane,
                     [&](double x, int64_t id, int32_t row) { cap_list_insert(l, cap_rank_key(x, id, row)); });
    cap_merge_sublanes<G>(l);
    if (FUSED) {
        cap_mark_rows<G>(cap_list_threshold(l), sorted, pos, len, n, xt, node_id, live_lane);
    } else if ((int)threadIdx.x < G) {
        const size_t base = ((size_t)tile * nlist + j) * (size_t)m * G + col;
#pragma unroll
        for (int i = 0; i < CAP_MAX; ++i)
            if (i >= CAP_MAX - m) {
                const size_t at = base + (size_t)(i - (CAP_MAX - m)) * G;
                part_hi[at] = l.k[i].hi, part_lo[at] = l.k[i].lo, part_rw[at] = l.k[i].rw;
            }
    }
}

// One wave per (multi-chunk segment blockIdx.x, tile blockIdx.y): the sub-lanes take the segment's chunks in turn, their
// lists merge, thr[tile][segment][column] = the m-th best key of the segment's column
template <int G>
__global__ __launch_bounds__(WAVE) void k_cap_merge(int32_t m, int32_t nmulti, int32_t nmseg, const int32_t *__restrict__ mseg_first,
                                                    const int32_t *__restrict__ mseg_count, const uint64_t *__restrict__ part_hi,
                                                    const uint64_t *__restrict__ part_lo, const uint32_t *__restrict__ part_rw,
                                                    uint64_t *__restrict__ thr_hi, uint64_t *__restrict__ thr_lo,
                                                    uint32_t *__restrict__ thr_rw)
{
    constexpr int R = WAVE / G;
    const int32_t ms = blockIdx.x, tile = blockIdx.y;
    if (ms >= nmseg) return;
    const int col = (int)threadIdx.x % G, sub = (int)threadIdx.x / G;
    const int32_t first = mseg_first[ms], cnt = mseg_count[ms];
    CapList l;
    cap_list_init(l, m);
    for (int32_t c = sub; c < cnt; c += R) {
        if (first + c >= nmulti) break;
        const size_t base = ((size_t)tile * nmulti + first + c) * (size_t)m * G + col;
        CapList other;
        cap_list_init(other, m);
#pragma unroll
        for (int i = 0; i < CAP_MAX; ++i)
            if (i >= CAP_MAX - m) {
                const size_t at = base + (size_t)(i - (CAP_MAX - m)) * G;
                other.k[i] = CapKey{part_hi[at], part_lo[at], part_rw[at]};
            }
        cap_list_merge(l, other);
    }
    cap_merge_sublanes<G>(l);
    if ((int)threadIdx.x < G) {
        const size_t at = ((size_t)tile * nmseg + ms) * G + col;
        const CapKey &t = cap_list_threshold(l);
        thr_hi[at] = t.hi, thr_lo[at] = t.lo, thr_rw[at] = t.rw;
    }
}

// One wave per (multi-chunk segment's chunk multi[blockIdx.x], tile blockIdx.y): the marking pass, in a launch of its own
template <int G>
__global__ __launch_bounds__(WAVE) void k_cap_mark(int32_t n, int32_t nmulti, int32_t nmseg, const int32_t *__restrict__ multi,
                                                   const int32_t *__restrict__ multi_mseg, const int32_t *__restrict__ chunk_pos,
                                                   const int32_t *__restrict__ chunk_len, const uint64_t *__restrict__ sorted,
                                                   const int64_t *__restrict__ node_id, const int32_t *__restrict__ slot_k, double *X,
                                                   const uint64_t *__restrict__ thr_hi, const uint64_t *__restrict__ thr_lo,
                                                   const uint32_t *__restrict__ thr_rw)
{
    const int32_t j = blockIdx.x, tile = blockIdx.y;
    if (j >= nmulti) return;
    const int32_t c = multi[j], ms = multi_mseg[j];
    if (ms < 0 || ms >= nmseg) return;
    const int col = (int)threadIdx.x % G;
    const bool live_lane = slot_k[(size_t)tile * G + col] >= 0;
    double *xt = X + (size_t)tile * (size_t)n * G + col;
    const size_t at = ((size_t)tile * nmseg + ms) * G + col;
    const CapKey thr{thr_hi[at], thr_lo[at], thr_rw[at]};
    cap_mark_rows<G>(thr, sorted, chunk_pos[c], chunk_len[c], n, xt, node_id, live_lane);
}

// ---- per call -------------------------------------------------------------------------------------------------------------------

template <class T>
static int32_t cap_upload(DevBuf<T> &d, const std::vector<T> &h, hipStream_t s)
{
    if (h.empty()) return RWR_OK;
    RWR_TRY(d.alloc(h.size()));
    RWR_HIP(hipMemcpyAsync(d.p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, s));
    return RWR_OK;
}

// RWR_CAP_CHUNK selects a smaller chunk (a selector between equivalent correct paths, for the parity test of
// the split form on small graphs); read per call, values outside [1, CAP_CHUNK] are ignored
static int32_t cap_chunk_rows()
{
    const char *e = getenv("RWR_CAP_CHUNK");
    const long v = e ? atol(e) : 0;
    return v >= 1 && v <= CAP_CHUNK ? (int32_t)v : CAP_CHUNK;
}

int32_t cap_build(rwr_graph *g, GroupCap &c, const int32_t *rows, int32_t nrows, int G, int tiles_max, Profile &prof)
{
    hipStream_t s = g->stream;
    const int32_t n = g->n;
    c.chunk = cap_chunk_rows();
    c.tiles = tiles_max;
    c.nkeys = 0, c.sorted = nullptr, c.plan = CapPlan{};
    int32_t max_label = 0;
    for (int32_t i = 0; i < n; ++i) max_label = c.group_of[i] > max_label ? c.group_of[i] : max_label;
    const int32_t nb = cand_blocks(nrows);
    RWR_TRY(c.d_label.alloc((size_t)n));
    RWR_TRY(c.d_off.alloc((size_t)nb + 1));
    std::vector<int32_t> start;
    return idle_on_error(s, [&]() -> int32_t {
        hipEvent_t a; RWR_TRY(prof.record(a, s));
        // 1. the labelled rows of the list as keys, in the list's order
        if (n > 0) RWR_HIP(hipMemcpyAsync(c.d_label.p, c.group_of, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
        if (nb > 0)
            hipLaunchKernelGGL(k_cap_count<CAP_ITEM_LABELLED>, dim3((unsigned)nb), dim3(CAND_BLOCK), 0, s, nrows, n, rows, c.d_label.p,
                               (const uint64_t *)nullptr, c.d_off.p);
        launch_cand_scan(nb, c.d_off.p, s);
        RWR_HIP(hipGetLastError());
        int32_t total = 0;
        RWR_HIP(hipMemcpyAsync(&total, c.d_off.p + nb, sizeof(int32_t), hipMemcpyDeviceToHost, s));
        RWR_HIP(hipStreamSynchronize(s));
        if (total < 0 || total > nrows) { set_error("group cap: %d labelled rows of %d", total, nrows); return RWR_E_HIP; }
        if (total > 0) {
            RWR_TRY(c.keys.alloc((size_t)total));
            RWR_TRY(c.keys_alt.alloc((size_t)total));
            RWR_TRY(c.vals.alloc((size_t)total));
            RWR_TRY(c.vals_alt.alloc((size_t)total));
            RWR_TRY(c.sort_temp.alloc(radix_sort_temp_bytes((size_t)total, 1)));
            hipLaunchKernelGGL(k_cap_scatter<CAP_ITEM_LABELLED>, dim3((unsigned)nb), dim3(CAND_BLOCK), 0, s, nrows, n, rows, c.d_label.p,
                               (const uint64_t *)nullptr, c.d_off.p, total, c.keys.p, c.vals.p, (int32_t *)nullptr);
            RWR_HIP(hipGetLastError());
            // 2. groups contiguous, rows ascending inside a group
            bool in_alt = false;
            RWR_TRY(radix_sort_pairs<uint64_t>(c.keys.p, c.keys_alt.p, c.vals.p, c.vals_alt.p, (size_t)total, 1, cap_key_bits(max_label),
                                               c.sort_temp.p, s, &in_alt));
            c.sorted = in_alt ? c.keys_alt.p : c.keys.p;
            c.nkeys = total;
            // 3. the segment heads, compacted the same way and read back once
            const int32_t nbh = cand_blocks(total);
            RWR_TRY(c.d_off.ensure((size_t)nbh + 1));            // (nbh <= nb: the stream has read the first table)
            hipLaunchKernelGGL(k_cap_count<CAP_ITEM_HEAD>, dim3((unsigned)nbh), dim3(CAND_BLOCK), 0, s, total, n, (const int32_t *)nullptr,
                               (const int32_t *)nullptr, c.sorted, c.d_off.p);
            launch_cand_scan(nbh, c.d_off.p, s);
            RWR_HIP(hipGetLastError());
            int32_t nseg = 0;
            RWR_HIP(hipMemcpyAsync(&nseg, c.d_off.p + nbh, sizeof(int32_t), hipMemcpyDeviceToHost, s));
            RWR_HIP(hipStreamSynchronize(s));
            if (nseg < 1 || nseg > total) { set_error("group cap: %d segments of %d keys", nseg, total); return RWR_E_HIP; }
            RWR_TRY(c.d_start.alloc((size_t)nseg));
            hipLaunchKernelGGL(k_cap_scatter<CAP_ITEM_HEAD>, dim3((unsigned)nbh), dim3(CAND_BLOCK), 0, s, total, n,
                               (const int32_t *)nullptr, (const int32_t *)nullptr, c.sorted, c.d_off.p, nseg, (uint64_t *)nullptr,
                               (uint32_t *)nullptr, c.d_start.p);
            RWR_HIP(hipGetLastError());
            start.resize((size_t)nseg + 1);
            RWR_HIP(hipMemcpyAsync(start.data(), c.d_start.p, (size_t)nseg * sizeof(int32_t), hipMemcpyDeviceToHost, s));
            RWR_HIP(hipStreamSynchronize(s));
            start[(size_t)nseg] = total;
            for (int32_t q = 0; q < nseg; ++q)
                if (start[(size_t)q] < 0 || start[(size_t)q] >= start[(size_t)q + 1]) {
                    set_error("group cap: segment heads out of order at %d", q);
                    return RWR_E_HIP;
                }
            c.plan = cap_plan(start.data(), nseg, c.m, c.chunk);
        }
        const CapPlan &pl = c.plan;
        RWR_TRY(cap_upload(c.d_chunk_pos, pl.chunk_pos, s));
        RWR_TRY(cap_upload(c.d_chunk_len, pl.chunk_len, s));
        RWR_TRY(cap_upload(c.d_single, pl.single, s));
        RWR_TRY(cap_upload(c.d_multi, pl.multi, s));
        RWR_TRY(cap_upload(c.d_multi_mseg, pl.multi_mseg, s));
        RWR_TRY(cap_upload(c.d_mseg_first, pl.mseg_first, s));
        RWR_TRY(cap_upload(c.d_mseg_count, pl.mseg_count, s));
        if (!pl.multi.empty()) {
            const size_t lists = (size_t)tiles_max * pl.multi.size() * (size_t)c.m * G;
            const size_t thrs = (size_t)tiles_max * pl.mseg_first.size() * G;
            RWR_TRY(c.part_hi.alloc(lists));
            RWR_TRY(c.part_lo.alloc(lists));
            RWR_TRY(c.part_rw.alloc(lists));
            RWR_TRY(c.thr_hi.alloc(thrs));
            RWR_TRY(c.thr_lo.alloc(thrs));
            RWR_TRY(c.thr_rw.alloc(thrs));
        }
        RWR_TRY(prof.end(prof.rank, a, s));
        RWR_HIP(hipStreamSynchronize(s));                        // (the plan's host vectors are pageable)
        return RWR_OK;
    });
}

// ---- per tile group ---------------------------------------------------------------------------------------------------------------

int32_t cap_group(rwr_graph *g, GroupCap &c, int G, int tg, const int32_t *slot_k, double *X, hipStream_t s)
{
    const CapPlan &pl = c.plan;
    const int32_t nsingle = (int32_t)pl.single.size(), nmulti = (int32_t)pl.multi.size(), nmseg = (int32_t)pl.mseg_first.size();
    if (tg < 1 || tg > c.tiles) { set_error("group cap: a tile group of %d tiles, planned for %d", tg, c.tiles); return RWR_E_HIP; }
    if (nsingle > 0)
        RWR_DISPATCH_G(G, hipLaunchKernelGGL((k_cap_select<GG, true>), dim3((unsigned)nsingle, (unsigned)tg), dim3(WAVE), 0, s, g->n, c.m,
                                              nsingle, c.d_single.p, c.d_chunk_pos.p, c.d_chunk_len.p, c.sorted, g->node_id.p, slot_k, X,
                                              (uint64_t *)nullptr, (uint64_t *)nullptr, (uint32_t *)nullptr));
    if (nmulti > 0) {
        RWR_DISPATCH_G(G, hipLaunchKernelGGL((k_cap_select<GG, false>), dim3((unsigned)nmulti, (unsigned)tg), dim3(WAVE), 0, s, g->n, c.m,
                                              nmulti, c.d_multi.p, c.d_chunk_pos.p, c.d_chunk_len.p, c.sorted, g->node_id.p, slot_k, X,
                                              c.part_hi.p, c.part_lo.p, c.part_rw.p));
        RWR_DISPATCH_G(G, hipLaunchKernelGGL((k_cap_merge<GG>), dim3((unsigned)nmseg, (unsigned)tg), dim3(WAVE), 0, s, c.m, nmulti, nmseg,
                                              c.d_mseg_first.p, c.d_mseg_count.p, c.part_hi.p, c.part_lo.p, c.part_rw.p, c.thr_hi.p,
                                              c.thr_lo.p, c.thr_rw.p));
        RWR_DISPATCH_G(G, hipLaunchKernelGGL((k_cap_mark<GG>), dim3((unsigned)nmulti, (unsigned)tg), dim3(WAVE), 0, s, g->n, nmulti, nmseg,
                                              c.d_multi.p, c.d_multi_mseg.p, c.d_chunk_pos.p, c.d_chunk_len.p, c.sorted, g->node_id.p,
                                              slot_k, X, c.thr_hi.p, c.thr_lo.p, c.thr_rw.p));
    }
    RWR_HIP(hipGetLastError());
    return RWR_OK;
}

}  // namespace rwr
