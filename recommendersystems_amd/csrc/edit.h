// What the edits of a resident graph share (internal; append.hip, remove.hip, node_remove.hip: DESIGN §3.11, §3.13, §3.23, §3.24):
// the NEW buffers an edit fills while the handle still holds the old ones, and how the handle takes them.  The two-phase rule
// is the drivers': alloc() belongs to phase 1, where a failure leaves the graph as it was; take() to phase 2, behind
// *swapped = true, and only exchanges pointers -- nothing in it can fail.  The old blocks go back to the block cache when the
// edit's locals go out of scope.
#pragma once
#include "engine.h"

namespace rwr {

// the raw link arrays of m links (w_norm_raw is never copied: the re-derive writes all of it)
struct StagedLinks {
    DevBuf<int32_t> dst;
    DevBuf<uint8_t> etype;
    DevBuf<double> w_raw, w_norm_raw;
    int32_t alloc(size_t m)
    {
        RWR_TRY(dst.alloc(m));
        RWR_TRY(etype.alloc(m));
        RWR_TRY(w_raw.alloc(m));
        return w_norm_raw.alloc(m);
    }
    void take(rwr_graph *g)
    {
        swap_blocks(g->dst, dst);
        swap_blocks(g->etype, etype);
        swap_blocks(g->w_raw, w_raw);
        swap_blocks(g->w_norm_raw, w_norm_raw);
    }
};

// The node-sized arrays of n nodes: the node SoA, which the edit fills, and every n-sized array the re-derive writes (it fills
// them whole, as the first build does with its own fresh allocations); with_item_lists: the two ITEM orders of n_items rows as
// well.  An append without a new ITEM leaves the resident lists alone; a removal always replaces them.
struct StagedNodes {
    DevBuf<int64_t> node_id, in_ptr;
    DevBuf<uint8_t> node_type, dangling;
    DevBuf<double> w_src;
    DevBuf<int32_t> row_order, row_order_x, item_rows, item_order;
    bool item_lists = false;
    int32_t alloc(size_t n, size_t n_items, bool with_item_lists)
    {
        item_lists = with_item_lists;
        RWR_TRY(node_id.alloc(n));
        RWR_TRY(node_type.alloc(n));
        RWR_TRY(dangling.alloc(n));
        RWR_TRY(w_src.alloc(n));
        RWR_TRY(in_ptr.alloc(n + 1));
        RWR_TRY(row_order.alloc(n));
        RWR_TRY(row_order_x.alloc(n));
        if (!item_lists) return RWR_OK;
        RWR_TRY(item_rows.alloc(n_items));
        return item_order.alloc(n_items);
    }
    void take(rwr_graph *g)
    {
        swap_blocks(g->node_id, node_id);
        swap_blocks(g->node_type, node_type);
        swap_blocks(g->dangling, dangling);
        swap_blocks(g->w_src, w_src);
        swap_blocks(g->in_ptr, in_ptr);
        swap_blocks(g->row_order, row_order);
        swap_blocks(g->row_order_x, row_order_x);
        if (!item_lists) return;
        swap_blocks(g->item_rows, item_rows);
        swap_blocks(g->item_order, item_order);
    }
};

// Nothing cached for the old node set survives an edit of the nodes: the list a single-seed call left in pinned memory, and a
// row-partitioned run (the re-derive ends it; its slab and seeds go too, so that only rwr_part_begin restarts it).
// cand_lists: the candidate lists as well.  Their validity test is the node count alone (cand_plan.h), which an append keeps
// sound -- it only adds rows behind the last one -- and a removal does not: a later rwr_graph_append_nodes can bring n back to
// a cached value over other rows.
inline void forget_node_set(rwr_graph *g, bool cand_lists)
{
    if (cand_lists)
        for (int e = 0; e < CAND_CACHE; ++e) {
            g->cand_entry[e] = CandEntry{};
            g->cand_rows[e].release();
        }
    g->sm_pin_count = -1;
    g->part_lo = g->part_hi = g->part_K = g->part_steps = 0;
    g->part_seeds.clear();
}

}  // namespace rwr
