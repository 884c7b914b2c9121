// What the kernels of rank.hip and rank_fused.hip share (device side): the geometry of the radix select, the 128-bit
// (score, id) key of a candidate, and the one sort-and-emit every LDS-sorted list goes out through.
#pragma once
#include "common.h"

namespace rwr {

constexpr int SEL_MAX_K = 1024;
constexpr int SEL_CAP = 3072;
constexpr int SEL_SLOTS = 4096;      // >= SEL_MAX_K - 1 + SEL_CAP
constexpr int SEL_LEVELS = 16;
constexpr int SEL_ROWS_PER_BLOCK = 4096;
constexpr int SEL_FUSED_LEVELS = 3;  // few seeds: levels decided by the histogram kernel's last workgroup (rank_group_select)

// hi = f64_orderable(score), lo = i64_orderable(id); {0, 0} lies below every real key (scores are >= +0.0: hi >= 2^63)
struct SelCand {
    uint64_t hi, lo;
};
__device__ __forceinline__ void sel_decode(const SelCand &v, int64_t *id, double *score)
{
    *id = (int64_t)(v.lo ^ 0x8000000000000000ull);
    const uint64_t u = (v.hi & 0x8000000000000000ull) ? (v.hi ^ 0x8000000000000000ull) : ~v.hi;
    double s;
    __builtin_memcpy(&s, &u, 8);
    *score = s;
}

__device__ __forceinline__ bool sel_lt(const SelCand &a, const SelCand &b) { return (a.hi < b.hi) || (a.hi == b.hi && a.lo < b.lo); }

// ... with the candidate's row (explain.hip): among equal (score, id) pairs the smaller row ranks first, which
// makes the order total.  {0, 0, 0x7FFFFFFF} lies below every real key
struct SelCandRow {
    uint64_t hi, lo;
    int32_t row, pad;
};
__device__ __forceinline__ bool sel_lt(const SelCandRow &a, const SelCandRow &b)
{
    return a.hi != b.hi ? a.hi < b.hi : a.lo != b.lo ? a.lo < b.lo : a.row > b.row;
}

// The state of one segment's radix select (rank.hip: the levels that fix it; the collects read it as their threshold)
struct SelState {
    uint64_t ph, pl;     // prefix: nbits <= 64: ph holds the top nbits of the score key (right-aligned);
                         // nbits > 64: ph = full score key, pl = top (nbits-64) bits of the id key
    int32_t nbits;       // bits decided so far
    int32_t k_rem;       // entries still to take from inside the prefix bin
    int32_t total;       // candidates of the segment (set at level 0)
    int32_t done;
    int32_t cand_cnt;    // collect cursor
    int32_t pad;
};

__device__ static inline int sel_cmp(uint64_t hi, uint64_t lo, const SelState &st)
{
    if (st.nbits == 0) return 0;
    if (st.nbits <= 64) {
        const uint64_t a = hi >> (64 - st.nbits);
        return a > st.ph ? 1 : (a < st.ph ? -1 : 0);
    }
    if (hi != st.ph) return hi > st.ph ? 1 : -1;
    const uint64_t b = lo >> (128 - st.nbits);
    return b > st.pl ? 1 : (b < st.pl ? -1 : 0);
}

// the workgroup's N2 (a power of two) entries of sc sorted descending by sel_lt (bitonic).  The caller has synchronised after filling sc
template <class C>
__device__ __forceinline__ void sel_sort(C *sc, int N2)
{
    for (int size = 2; size <= N2; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = threadIdx.x; t < N2 / 2; t += blockDim.x) {
                const int lo_i = 2 * t - (t & (stride - 1));
                const int hi_i = lo_i + stride;
                const bool desc = (lo_i & size) == 0;        // first half of each bitonic pair: descending
                const C a = sc[lo_i], b = sc[hi_i];
                const bool a_lt_b = sel_lt(a, b);
                if (a_lt_b == desc) {
                    sc[lo_i] = b;
                    sc[hi_i] = a;
                }
            }
            __syncthreads();
        }
    }
}
// the first min(cnt, top_n) entries of the sorted sc go out as row orow of the result tables
__device__ __forceinline__ void sel_emit(const SelCand *sc, int cnt, int32_t orow, int32_t top_n, int64_t *__restrict__ out_id,
                                         double *__restrict__ out_score, int32_t *__restrict__ out_counts)
{
    int take = cnt < top_n ? cnt : top_n;
    if (threadIdx.x == 0) out_counts[orow] = take;
    for (int i = threadIdx.x; i < take; i += blockDim.x)
        sel_decode(sc[i], &out_id[(size_t)orow * top_n + i], &out_score[(size_t)orow * top_n + i]);
}
__device__ __forceinline__ void sel_sort_emit(SelCand *sc, int N2, int cnt, int32_t orow, int32_t top_n, int64_t *__restrict__ out_id,
                                              double *__restrict__ out_score, int32_t *__restrict__ out_counts)
{
    sel_sort(sc, N2);
    sel_emit(sc, cnt, orow, top_n, out_id, out_score, out_counts);
}

}  // namespace rwr
