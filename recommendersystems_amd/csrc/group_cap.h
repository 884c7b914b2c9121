// A diversity cap on the ranked walks (internal; group_cap.hip): at most m candidates per caller-set group of
// nodes in every seed's list.  One more stage of the ranked end: after the exclusion and the deny marks, before the
// destination, the cells of the candidates outside their group's best m of a column receive -1.
#pragma once
#include "cap_plan.h"
#include "iterate.h"

namespace rwr {

// The cap of one call.  The object is declared before the driver's StreamsIdle (ranked_end.h's lifetime rule): its device
// buffers outlive the kernels that read them, on error paths too.
struct GroupCap {
    const int32_t *group_of = nullptr;     // host, n labels as typed_call_check passed them; < 0: the node is never capped
    int32_t m = 0;                         // group_cap, in [1, CAP_MAX]

    // cap_build: the sorted keys of the call's labelled candidates and cap_plan.h's tables over them
    int32_t chunk = CAP_CHUNK;
    const uint64_t *sorted = nullptr;      // keys.p or keys_alt.p, whichever the sort ended in
    int32_t nkeys = 0;
    CapPlan plan;
    int32_t tiles = 0;                     // tiles a group holds at most: the partial lists' and thresholds' extent
    DevBuf<int32_t> d_label, d_off, d_start;
    DevBuf<uint64_t> keys, keys_alt;
    DevBuf<uint32_t> vals, vals_alt;
    DevBuf<uint8_t> sort_temp;
    DevBuf<int32_t> d_chunk_pos, d_chunk_len, d_single, d_multi, d_multi_mseg, d_mseg_first, d_mseg_count;
    DevBuf<uint64_t> part_hi, part_lo, thr_hi, thr_lo;   // [tile][multi chunk][m][G] lists, [tile][multi segment][G] thresholds
    DevBuf<uint32_t> part_rw, thr_rw;
};

// From the call's ascending candidate list `rows` (device; the call's own or the handle's cached one, which is only read):
// keys, sort, segment heads, one read-back of the head positions, the tables.  G: the call's tile width, tiles_max: an upper
// bound of its tile group.  Call it on an idle stream and before the workspace is sized; the stream is idle on return.
// Booked as prof.rank.
int32_t cap_build(rwr_graph *g, GroupCap &c, const int32_t *rows, int32_t nrows, int G, int tiles_max, Profile &prof);
// The marking of one tile group (tg tiles of G slots, slot_k their liveness) on s; nothing is launched without planned chunks
int32_t cap_group(rwr_graph *g, GroupCap &c, int G, int tg, const int32_t *slot_k, double *X, hipStream_t s);

}  // namespace rwr
