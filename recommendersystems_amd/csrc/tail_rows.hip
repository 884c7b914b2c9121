// The row lists of a batch's last steps, derived from the built matrix on first use: tail_rows_prepare.
#include "engine.h"

#include <vector>
#include <cstdlib>

namespace rwr {

// flag every source of an explicit link into a row of the previous level, one wave per row of that level walking its
// transposed in-list -- the entries the SpMM gathers for that row
__global__ __launch_bounds__(256) void k_tail_flag(int32_t nrows, const int32_t *__restrict__ rows,
                                                   const int64_t *__restrict__ in_ptr, const int32_t *__restrict__ in_src,
                                                   uint8_t *__restrict__ flag)
{
    const int64_t q = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
    if (q >= nrows) return;
    const int lane = threadIdx.x & (WAVE - 1);
    const int32_t j = rows[q];
    const int64_t p1 = in_ptr[j + 1];
    for (int64_t p = in_ptr[j] + lane; p < p1; p += WAVE) flag[in_src[p]] = 1;
}
// ... the keys of a stable one-bit partition of row_order: rows whose flag equals `match` first; *count = how many, *links =
// their in-links (what a launch over them gathers)
__global__ __launch_bounds__(256) void k_tail_keys(int32_t n, const int32_t *__restrict__ row_order,
                                                   const uint8_t *__restrict__ flag, uint8_t match,
                                                   uint32_t *__restrict__ key, uint32_t *__restrict__ val, int *__restrict__ count,
                                                   const int64_t *__restrict__ in_ptr, unsigned long long *__restrict__ links)
{
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    bool in = false;
    unsigned long long deg = 0;
    if (r < n) {
        const int32_t i = row_order[r];
        in = flag[i] == match;
        key[r] = in ? 0u : 1u;
        val[r] = (uint32_t)i;
        if (in) deg = (unsigned long long)(in_ptr[i + 1] - in_ptr[i]);
    }
    const unsigned long long b = __ballot(in);
    for (int off = WAVE / 2; off > 0; off >>= 1) deg += __shfl_down(deg, off, WAVE);
    if ((threadIdx.x & (WAVE - 1)) == 0 && b) {
        atomicAdd(count, (int)__popcll(b));
        atomicAdd(links, deg);
    }
}
// ... and the seed-row flag of step T - 1: node s has an explicit raw link into an ITEM row that is not also the target of
// one of its raw LIKE links.  Only such a link carries s's rank at step T - 1 into a row the ranking reads: k_exclude drops
// the targets of the LIKE links, and UNDEFINED links are no matrix entries.  One wave per node; a node with more than
// TAIL_SCAN_MAX raw links is flagged without the pairwise search (a flag that need not be set only costs a chain)
constexpr int64_t TAIL_SCAN_MAX = 4096;
__global__ __launch_bounds__(256) void k_tail_seed_flag(int32_t n, const int64_t *__restrict__ rowptr,
                                                        const int32_t *__restrict__ dst, const uint8_t *__restrict__ etype,
                                                        const uint8_t *__restrict__ node_type, uint8_t *__restrict__ flag)
{
    const int64_t s = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
    if (s >= n) return;
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t p0 = rowptr[s], p1 = rowptr[s + 1];
    bool reach = false;
    for (int64_t p = p0 + lane; p < p1; p += WAVE) {
        const uint8_t ty = etype[p];
        const int32_t t = dst[p];
        if (ty == RWR_EDGE_UNDEFINED || ty == RWR_EDGE_LIKE || t < 0 || t >= n || node_type[t] != RWR_NODE_ITEM) continue;
        bool liked = false;
        if (p1 - p0 <= TAIL_SCAN_MAX)
            for (int64_t q = p0; q < p1 && !liked; ++q) liked = etype[q] == RWR_EDGE_LIKE && dst[q] == t;
        reach = reach || !liked;
    }
    if (__ballot(reach) && lane == 0) flag[s] = 1;
}

// Every list is a stable one-bit partition of row_order, so that it keeps its in-degree-descending load balance; with them
// come the per-node chain flags of those steps.
// Level k >= 2 is built only while a launch over it gathers at most 80 % of the matrix: past that it costs what a full launch
// costs, and every deeper level walks at least as much on the graphs that get that far.  RWR_TAIL_DEPTH caps the levels.
int32_t tail_rows_prepare(rwr_graph *g)
{
    if (g->tail_state == 1) return RWR_OK;
    g->bound_first = -1;
    static const int depth_env = [] {
        const char *e = getenv("RWR_TAIL_DEPTH");
        const int v = e ? atoi(e) : rwr_graph::TAIL_MAX;
        return v < 1 ? 1 : v > rwr_graph::TAIL_MAX ? rwr_graph::TAIL_MAX : v;
    }();
    const int32_t n = g->n;
    hipStream_t s = g->stream;
    DevBuf<uint8_t> flag, temp;
    DevBuf<uint32_t> key, key2, val, val2;
    DevBuf<int> cnt;
    DevBuf<unsigned long long> links;
    const size_t nn = (size_t)(n > 0 ? n : 1);
    RWR_TRY(flag.alloc(nn));
    RWR_TRY(key.alloc(nn));
    RWR_TRY(key2.alloc(nn));
    RWR_TRY(val.alloc(nn));
    RWR_TRY(val2.alloc(nn));
    RWR_TRY(cnt.alloc(1));
    RWR_TRY(links.alloc(1));
    RWR_TRY(temp.alloc(radix_sort_temp_bytes(nn, 1)));
    std::vector<uint8_t> h_flag((size_t)n);
    g->h_tail_flag.assign((size_t)n, 0);
    for (int32_t i = 0; i < n; ++i) g->h_tail_flag[i] = g->h_is_item[i];   // bit 0: the last step's chain of an ITEM seed
    if (depth_env >= 2 && n > 0) {   // bit 1
        RWR_HIP(hipMemsetAsync(flag.p, 0, nn, s));
        hipLaunchKernelGGL(k_tail_seed_flag, dim3(cdiv((size_t)n, 256 / WAVE)), dim3(256), 0, s, n, g->rowptr.p, g->dst.p,
                           g->etype.p, g->node_type.p, flag.p);
        RWR_HIP(hipMemcpyAsync(h_flag.data(), flag.p, (size_t)n, hipMemcpyDeviceToHost, s));
        RWR_HIP(hipStreamSynchronize(s));
        for (int32_t i = 0; i < n; ++i) g->h_tail_flag[i] |= (uint8_t)(h_flag[i] << 1);
    }
    g->tail_depth = 0;
    for (int l = 0; l < depth_env; ++l) {
        int h_cnt = 0;
        unsigned long long h_links = 0;
        if (n > 0) {
            if (l > 0) {   // the sources of the previous level's in-links
                RWR_HIP(hipMemsetAsync(flag.p, 0, nn, s));
                if (g->tail_n[l - 1] > 0)
                    hipLaunchKernelGGL(k_tail_flag, dim3(cdiv((size_t)g->tail_n[l - 1], 256 / WAVE)), dim3(256), 0, s,
                                       g->tail_n[l - 1], g->tail_rows[l - 1].p, g->in_ptr.p, g->in_src.p, flag.p);
            }
            RWR_HIP(hipMemsetAsync(cnt.p, 0, sizeof(int), s));
            RWR_HIP(hipMemsetAsync(links.p, 0, sizeof(unsigned long long), s));
            hipLaunchKernelGGL(k_tail_keys, dim3(cdiv((size_t)n, 256)), dim3(256), 0, s, n, g->row_order.p,
                               l == 0 ? g->node_type.p : flag.p, (uint8_t)(l == 0 ? RWR_NODE_ITEM : 1), key.p, val.p, cnt.p,
                               g->in_ptr.p, links.p);
            RWR_HIP(hipMemcpyAsync(&h_cnt, cnt.p, sizeof(int), hipMemcpyDeviceToHost, s));
            RWR_HIP(hipMemcpyAsync(&h_links, links.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
            RWR_HIP(hipStreamSynchronize(s));
            if (l >= 2 && h_links * 5 > (unsigned long long)g->nnz * 4) break;
            bool alt = false;
            RWR_TRY(radix_sort_pairs<uint32_t>(key.p, key2.p, val.p, val2.p, (size_t)n, 1, 1, temp.p, s, &alt));
            RWR_TRY(g->tail_rows[l].alloc((size_t)(h_cnt > 0 ? h_cnt : 1)));
            launch_u32_to_i32(alt ? val2.p : val.p, g->tail_rows[l].p, h_cnt, s);
            if (l >= 2) {   // bit l: the seed row is a source of level l - 1, whose rows step T - l + 1 produces
                RWR_HIP(hipMemcpyAsync(h_flag.data(), flag.p, (size_t)n, hipMemcpyDeviceToHost, s));
                RWR_HIP(hipStreamSynchronize(s));
                for (int32_t i = 0; i < n; ++i) g->h_tail_flag[i] |= (uint8_t)(h_flag[i] << l);
            }
        }
        g->tail_n[l] = h_cnt;
        g->tail_depth = l + 1;
    }
    for (int l = g->tail_depth; l < rwr_graph::TAIL_MAX; ++l) { g->tail_rows[l].release(); g->tail_n[l] = 0; }
    RWR_HIP(hipGetLastError());
    RWR_HIP(hipStreamSynchronize(s));   // the scratch buffers are released on return
    g->tail_state = 1;
    return RWR_OK;
}

}  // namespace rwr
