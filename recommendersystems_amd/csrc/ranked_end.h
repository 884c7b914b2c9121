// The ranked end of a batch (internal; ranked_end.hip): what the typed seed driver (typed.hip) and the
// restart-vector driver (restart_batch.hip) do with a tile group whose walks are finished.  The excluded elements of the
// group's X[tile][n][G] are marked with -1; then the candidates are ranked into K x top_n lists, evaluated against test
// sets by counting, or the test ids' positions in the whole lists are found by the same counting; after the last group the
// result is copied back once.  Three independent descriptions say which end: the candidates, the exclusion, the destination;
// the filtered entries add a fourth, the seeds' deny lists, the capped entries a fifth, the group cap, the explained entry a
// sixth, the reasons of the list's entries; the long entries name a fourth destination, lists beyond the select's limit.
//
// Lifetime: the object (and the EvalEnd or PosEnd it points to) is declared before the driver's StreamsIdle, so the device copies of
// its plans outlive the kernels that read them, on error paths too.
#pragma once
#include "eval_count.h"
#include "eval_pos.h"
#include "exclude_plan.h"
#include "member_plan.h"

namespace rwr {

struct Profile;   // iterate.h
struct GroupCap;  // group_cap.h
struct WhyEnd;    // explain.h
struct LongEnd;   // long_list.h

struct RankedEnd {
    const char *who = "";              // the entry point, for the messages
    // the candidates: a device row list (cand_rows_get's cached list of a node type); nullptr: the ITEM rows through the
    // ITEM rankers (rank_group, which picks select or sort by top_n)
    const int32_t *rows = nullptr;
    int32_t nrows = 0;
    // the exclusion: set k (CSR over batch positions) loses the targets of its members' raw links whose type has its bit in
    // mask and, with members, the members' own rows.  mask == 0 and !members: nothing is planned, nothing launched
    const int64_t *set_ptr = nullptr;
    const int32_t *set_idx = nullptr;
    uint32_t mask = 0;
    bool members = false;
    // sets of exactly one member per slot may name them by a device array over the slots instead (-1: a padding slot): the
    // members' rows are then marked from it and no pairs are planned or uploaded (measured)
    const int32_t *slot_member = nullptr;
    // the deny lists (the filtered entries): a second set description, independent of the one above -- set k
    // (CSR over batch positions, host) loses the rows deny_idx[deny_ptr[k] .. deny_ptr[k + 1]) themselves, whatever their
    // links or types; marked after the exclusion above, before the destination.  deny_ptr == nullptr: nothing is planned,
    // nothing launched
    const int64_t *deny_ptr = nullptr;
    const int32_t *deny_idx = nullptr;
    // the group cap (the capped entries): at most m candidates per caller-set group in every slot's list -- the
    // cells outside their group's best m of a column are marked after the deny lists, before the destination.  The driver
    // builds the object's tables (cap_build) once the candidate list exists.  nullptr: nothing is built, nothing launched
    GroupCap *cap = nullptr;
    // the destination: the caller's list tables, top_n wide, or (ev != nullptr) the evaluation records, or (pos != nullptr)
    // the positions and scores of the test ids; at most one of ev and pos is set
    int32_t top_n = 0;
    int64_t *ids = nullptr;
    double *scores = nullptr;
    int32_t *counts = nullptr;
    EvalEnd *ev = nullptr;
    PosEnd *pos = nullptr;
    // the reasons (the explained entry; the list destination only): the lists keep their entries' rows -- the
    // select's last two launches are explain.hip's row-carrying pair -- and every entry's best in-link addends over the
    // group's previous ranks are found after the ranking.  nullptr: the stock launches, nothing more
    WhyEnd *why = nullptr;
    // the long lists (the long entries; the list destination only, without reasons): top_n lies beyond the
    // select's limit -- long_list.hip's collect, run sort and merge passes write the lists, always with their entries' rows.
    // nullptr: top_n is within the select's limit
    LongEnd *lng = nullptr;

    // The zeroed output tables (or records) of the call and the plans of this slot assignment: slot_k[slot] = batch position,
    // -1 = padding; slots_per_group slots form a tile group.  The driver has put slot_k into g->d_slot_k -- the ranking's
    // output-row table and its liveness array (>= 0: a live slot).  The host vectors are pageable: the caller synchronises s.
    int32_t prepare(rwr_graph *g, int32_t K, const std::vector<int32_t> &slot_k, size_t slots_per_group, hipStream_t s);
    // Tile group grp (tg tiles of G slots from slot q0 on) holds its final ranks in X: the exclusion, then the ranking or
    // the evaluation, booked as prof.rank.  Y: the group's previous ranks (GroupIter's Y after the last step), which only `why`
    // reads
    int32_t finish_group(rwr_graph *g, int G, int tg, int grp, size_t q0, double *X, Profile &prof, hipStream_t s,
                         const double *Y = nullptr);
    // after the last group: K x top_n list entries, the K evaluation records, or the test ids' positions and scores
    int32_t copy_back(rwr_graph *g, int32_t K);

private:
    ExcludePlan plan;
    DevBuf<int32_t> d_seg_slot;
    DevBuf<int64_t> d_seg_p0, d_seg_p1;
    MemberPlan mplan;
    DevBuf<int32_t> d_pair_slot, d_pair_row;
    MemberPlan dplan;                  // the deny lists' (slot, row) pairs
    DevBuf<int32_t> d_deny_slot, d_deny_row;
};

}  // namespace rwr
