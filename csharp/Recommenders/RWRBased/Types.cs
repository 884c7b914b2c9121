// The two value types of the reference's public surface (Recommenders/RWRBased/Graph.cs:4-35), field for field: the
// unmodified host constructs them and reads/writes their public fields (DataLoader.cs:40,53,66,73,424;
// Experiment.cs:90-97), so names, field order and constructors are part of the drop-in contract.
namespace Recommenders.RWRBased {
    public struct Node {
        public long id;
        public NodeType type;
        public Node(long id) { this.id = id; this.type = NodeType.UNDEFINED; }
        public Node(long id, NodeType type) { this.id = id; this.type = type; }
    }

    public struct ForwardLink {
        public int targetNode;
        public EdgeType type;
        public double weight;
        public ForwardLink(int targetNode, double weight) { this.targetNode = targetNode; this.type = EdgeType.UNDEFINED; this.weight = weight; }
        public ForwardLink(int targetNode, EdgeType type, double weight) { this.targetNode = targetNode; this.type = type; this.weight = weight; }
    }

    // addition: rwr_stats (include/rwr.h), field for field -- the library's counters for a graph (Graph.Stats()).  The last seven
    // say which kernels served the single-seed SpMV steps and the source-block sweep's geometry (all 0: the graph does not take it)
    [System.Runtime.InteropServices.StructLayout(System.Runtime.InteropServices.LayoutKind.Sequential)]
    public struct RwrStats {
        public int struct_size, n;
        public long nnz_raw, nnz;
        public int uniform, tile_seeds, tile_group, mode;
        public double build_ms, spmm_ms;
        public long spmm_launches, spmm_seed_steps;
        public double chain_ms;
        public long chain_launches;
        public double rank_ms, iterate_wall_ms, total_wall_ms;
        public long seeds_done, chain_redo_blocks;
        public double spmm_dense_ms;
        public long spmm_dense_launches, spmm_dense_seed_steps;
        public int uniform_path, reserved1;
        public long frontier_list_launches, rank_fused_groups, rank_fused_fallbacks, rank_pruned_rows;
        public double rank_bound_ms;
        public long x_clear_skipped, entry_live_launches;
        public long spmv_sweep_launches, spmv_hub_launches, spmv_binned_launches;
        public int sweep_k, sweep_blocks, sweep_wgs, sweep_partial;
    }

}
