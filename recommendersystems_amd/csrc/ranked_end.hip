// The ranked end of a batch (ranked_end.h): the exclusion kernels, and the three operations around a driver's group loop.
#include "ranked_end.h"

#include "explain.h"
#include "group_cap.h"
#include "iterate.h"
#include "long_list.h"

namespace rwr {

// Recommender.cs:20-24 with the link type as a set, applied to every member of the slot's set: the targets of the members' RAW
// out-links whose type has its bit in `mask` are not candidates.  Marked by overwriting their (final) score with -1 -- valid
// scores are >= 0.  The members' raw lists arrive cut into segments of at most EXCLUDE_SEG_MAX links (exclude_plan.h); one
// wave per segment, the lanes at consecutive links.  Segments of one slot may name the same target (two members that like it,
// a member listed twice): every one of them stores the same -1; a target of another node type than the candidates' receives
// a -1 that nobody reads.  Link types are as unchecked as node types, so a raw link may carry any value up to 255: the mask
// has no bit for a type >= TYPED_EDGE_TYPES, such a link is never masked, and the test in front of the shift keeps the shift
// count below the mask's width.
__global__ __launch_bounds__(64) void k_exclude_typed(int32_t n, int G, int32_t nseg, const int32_t *__restrict__ seg_slot,
                                                      const int64_t *__restrict__ seg_p0, const int64_t *__restrict__ seg_p1,
                                                      const int32_t *__restrict__ dst, const uint8_t *__restrict__ etype,
                                                      uint32_t mask, double *__restrict__ X)
{
    const int32_t j = blockIdx.x;
    if (j >= nseg) return;
    const int32_t q = seg_slot[j];
    double *x = X + (size_t)(q / G) * (size_t)n * G + (q % G);
    const int64_t p1 = seg_p1[j];
    for (int64_t p = seg_p0[j] + threadIdx.x; p < p1; p += WAVE) {
        const uint32_t t = etype[p];                             // (unchecked at create: any value 0..255)
        if (t < TYPED_EDGE_TYPES && ((mask >> t) & 1u)) x[(size_t)dst[p] * G] = -1.0;
    }
}

// One thread per (slot, member) pair of the group (member_plan.h) marks the member's own row in its slot's column -- also of
// a member without raw links, which has no segment.  A member listed twice, or that is a masked target as well, simply
// receives its -1 twice.
__global__ __launch_bounds__(256) void k_exclude_members(int32_t n, int G, int32_t npairs, const int32_t *__restrict__ pair_slot,
                                                         const int32_t *__restrict__ pair_row, double *__restrict__ X)
{
    const int32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= npairs) return;
    const int32_t q = pair_slot[j], row = pair_row[j];
    if (row < 0 || row >= n) return;                             // (member_plan.h plans rows of [0, n) only)
    X[(size_t)(q / G) * (size_t)n * G + (size_t)row * G + (q % G)] = -1.0;
}

// ... and of sets of one member per slot, named by slot (RankedEnd::slot_member): one thread per slot
__global__ __launch_bounds__(64) void k_exclude_self(int32_t n, int G, int nslots, const int32_t *__restrict__ slot_member,
                                                     double *__restrict__ X)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nslots) return;
    const int32_t row = slot_member[q];
    if (row < 0 || row >= n) return;
    X[(size_t)(q / G) * (size_t)n * G + (size_t)row * G + (q % G)] = -1.0;
}

// a plan's host array into its device copy (nothing for an empty one)
template <class T>
static int32_t upload(DevBuf<T> &d, const std::vector<T> &h, hipStream_t s)
{
    if (h.empty()) return RWR_OK;
    RWR_TRY(d.alloc(h.size()));
    RWR_HIP(hipMemcpyAsync(d.p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, s));
    return RWR_OK;
}

int32_t RankedEnd::prepare(rwr_graph *g, int32_t K, const std::vector<int32_t> &slot_k, size_t slots_per_group, hipStream_t s)
{
    if (ev) RWR_TRY(eval_prepare(g, *ev, K, slot_k, slots_per_group, who, s));
    else if (pos) RWR_TRY(pos_prepare(g, *pos, K, slot_k, slots_per_group, who, s));
    else RWR_TRY(ensure_out_tables(g, K, top_n, s));
    if (why && !ev && !pos) RWR_TRY(why_prepare(g, *why, K, top_n, s));
    if (lng && !ev && !pos) RWR_TRY(long_prepare(g, *lng, K, top_n, s));
    if (mask != 0) {                                            // (mask 0 looks at no link)
        plan = exclude_plan(g->n, g->h_rowptr.data(), slot_k.size(), slot_k.data(), slots_per_group, K, set_ptr, set_idx);
        if (plan.check.verdict != EXCLUDE_OK) {                 // (api.hip refuses such sets before the call gets here)
            set_error("%s: exclusion sets failed their check (verdict %d)", who, (int)plan.check.verdict);
            return RWR_E_INVALID;
        }
        if (plan.seg_slot.size() > 0x7FFFFFFFull) { set_error("%s: too many exclusion segments", who); return RWR_E_UNSUPPORTED; }
        RWR_TRY(upload(d_seg_slot, plan.seg_slot, s));
        RWR_TRY(upload(d_seg_p0, plan.seg_p0, s));
        RWR_TRY(upload(d_seg_p1, plan.seg_p1, s));
    }
    if (members && !slot_member) {
        mplan = member_plan(g->n, slot_k.size(), slot_k.data(), slots_per_group, K, set_ptr, set_idx);
        if (mplan.check.verdict != EXCLUDE_OK) {
            set_error("%s: exclusion sets failed their check (verdict %d)", who, (int)mplan.check.verdict);
            return RWR_E_INVALID;
        }
        if (mplan.pair_slot.size() > 0x7FFFFFFFull) { set_error("%s: too many set members", who); return RWR_E_UNSUPPORTED; }
        RWR_TRY(upload(d_pair_slot, mplan.pair_slot, s));
        RWR_TRY(upload(d_pair_row, mplan.pair_row, s));
    }
    if (deny_ptr) {
        dplan = member_plan(g->n, slot_k.size(), slot_k.data(), slots_per_group, K, deny_ptr, deny_idx);
        if (dplan.check.verdict != EXCLUDE_OK) {                // (api.hip refuses such lists before the call gets here)
            set_error("%s: deny lists failed their check (verdict %d)", who, (int)dplan.check.verdict);
            return RWR_E_INVALID;
        }
        if (dplan.pair_slot.size() > 0x7FFFFFFFull) { set_error("%s: too many denied nodes", who); return RWR_E_UNSUPPORTED; }
        RWR_TRY(upload(d_deny_slot, dplan.pair_slot, s));
        RWR_TRY(upload(d_deny_row, dplan.pair_row, s));
    }
    return RWR_OK;
}

int32_t RankedEnd::finish_group(rwr_graph *g, int G, int tg, int grp, size_t q0, double *X, Profile &prof, hipStream_t s,
                                const double *Y)
{
    const int32_t *slot_k = g->d_slot_k.p + q0;                 // (the rankers read it for liveness as well: a sign test)
    hipEvent_t a; RWR_TRY(prof.record(a, s));
    if (mask != 0) {
        const int64_t j0 = plan.group_off[(size_t)grp], nseg = plan.group_off[(size_t)grp + 1] - j0;
        if (nseg > 0)
            hipLaunchKernelGGL(k_exclude_typed, dim3((unsigned)nseg), dim3(64), 0, s, g->n, G, (int32_t)nseg, d_seg_slot.p + j0,
                               d_seg_p0.p + j0, d_seg_p1.p + j0, g->dst.p, g->etype.p, mask, X);
    }
    if (members && slot_member) {
        hipLaunchKernelGGL(k_exclude_self, dim3(cdiv((size_t)tg * G, 64)), dim3(64), 0, s, g->n, G, tg * G, slot_member + q0, X);
    } else if (members) {
        const int64_t m0 = mplan.group_off[(size_t)grp], npairs = mplan.group_off[(size_t)grp + 1] - m0;
        if (npairs > 0)
            hipLaunchKernelGGL(k_exclude_members, dim3(cdiv((size_t)npairs, 256)), dim3(256), 0, s, g->n, G, (int32_t)npairs,
                               d_pair_slot.p + m0, d_pair_row.p + m0, X);
    }
    if (deny_ptr) {
        const int64_t m0 = dplan.group_off[(size_t)grp], npairs = dplan.group_off[(size_t)grp + 1] - m0;
        if (npairs > 0)
            hipLaunchKernelGGL(k_exclude_members, dim3(cdiv((size_t)npairs, 256)), dim3(256), 0, s, g->n, G, (int32_t)npairs,
                               d_deny_slot.p + m0, d_deny_row.p + m0, X);
    }
    RWR_HIP(hipGetLastError());
    if (cap) RWR_TRY(cap_group(g, *cap, G, tg, slot_k, X, s));
    if (ev) RWR_TRY(eval_group(g, *ev, G, tg, q0, X, rows ? rows : g->item_rows.p, rows ? nrows : g->n_items, s));
    else if (pos) RWR_TRY(pos_group(g, *pos, G, tg, q0, X, rows ? rows : g->item_rows.p, rows ? nrows : g->n_items, s));
    else if (lng) {                                             // (top_n beyond the select's limit: long_list.hip's entry)
        if (!rows || why) { set_error("%s: long lists need a candidate list and carry no reasons", who); return RWR_E_INVALID; }
        if (nrows > 0) RWR_TRY(long_rank_group(g, *lng, G, tg, slot_k, top_n, X, s, rows, nrows));
    }
    else if (why) {                                             // (a candidate list and top_n <= the select's limit: explain.hip's entry)
        if (!rows) { set_error("%s: reasons need a candidate list", who); return RWR_E_INVALID; }
        if (nrows > 0) {
            RWR_TRY(why_rank_group(g, *why, G, tg, slot_k, top_n, X, s, rows, nrows));
            RWR_TRY(why_group(g, *why, G, tg, slot_k, top_n, Y, s));
        }
    }
    else if (!rows) RWR_TRY(rank_group(g, G, tg, slot_k, slot_k, top_n, X, s));
    else if (nrows > 0) RWR_TRY(rank_group_select(g, G, tg, slot_k, top_n, X, slot_k, s, rows, nrows));   // (top_n <= its limit: api.hip)
    RWR_TRY(prof.end(prof.rank, a, s));                         // (no candidate: the zeroed tables stand)
    return RWR_OK;
}

int32_t RankedEnd::copy_back(rwr_graph *g, int32_t K)
{
    if (ev) return eval_copy_back(g, *ev, K, who, g->stream);
    if (pos) return pos_copy_back(g, *pos, K, who, g->stream);
    RWR_TRY(copy_lists_back(g, K, top_n, ids, scores, counts, top_n));
    if (lng) return long_copy_back(g, *lng, K, top_n);
    return why ? why_copy_back(g, *why, K, top_n) : RWR_OK;
}

}  // namespace rwr
