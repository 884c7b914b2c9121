// P/Invoke declarations of include/rwr.h.  Thin on purpose: every overload maps 1:1 onto a C entry point,
// and recommendersystems_amd/_lib.py (ctypes) binds the very same signatures and IS exercised by the tests.
// NOTE: there is no C# toolchain in the build image, so this shim is source only (INTEGRATION.md).
using System;
using System.Runtime.InteropServices;

namespace Recommenders.RWRBased {
    [StructLayout(LayoutKind.Sequential)]
    internal struct RwrOpts {
        public int struct_size, device, mode, tile_seeds, tile_group, profile;
        public long workspace_bytes;
        public int seed_row_kernel, reserved0;
    }

    // one graph of a rwr_eval_graphs batch: pointers to the caller's (pinned) arrays -- include/rwr.h: rwr_graph_desc
    [StructLayout(LayoutKind.Sequential)]
    internal struct RwrGraphDesc {
        public int n_nodes, reserved0;
        public IntPtr node_id, node_type, rowptr, dst, etype, w;
    }

    internal sealed class GraphHandle : SafeHandle {
        // the reference types have no Dispose(): native memory is released by the finalizer of this SafeHandle
        public GraphHandle() : base(IntPtr.Zero, true) { }
        public override bool IsInvalid { get { return handle == IntPtr.Zero; } }
        protected override bool ReleaseHandle() { Native.rwr_graph_destroy(handle); return true; }
    }

    internal static class Native {
        const string Lib = "rwr";   // librwr.so
        [DllImport(Lib)] public static extern IntPtr rwr_last_error();
        [DllImport(Lib)] public static extern int rwr_device_count();
        [DllImport(Lib)] public static extern int rwr_graph_create(int n, long[] node_id, byte[] node_type, long[] rowptr,
            int[] dst, byte[] etype, double[] w, ref RwrOpts opts, out GraphHandle g);
        [DllImport(Lib)] public static extern int rwr_graph_update_links(GraphHandle g, long count, long[] link_index,
            byte[] etype, double[] w);
        [DllImport(Lib)] public static extern int rwr_graph_append_links(GraphHandle g, long count, int[] src, int[] dst,
            byte[] etype, double[] w, long[] new_index_out);
        [DllImport(Lib)] public static extern int rwr_graph_append_nodes(GraphHandle g, int n_new, long[] node_id, byte[] node_type,
            long count, int[] src, int[] dst, byte[] etype, double[] w, long[] new_index_out);
        [DllImport(Lib)] public static extern int rwr_graph_remove_links(GraphHandle g, long count, long[] link_index);
        [DllImport(Lib)] public static extern int rwr_graph_remove_nodes(GraphHandle g, int count, int[] node_index, int[] new_node_index_out, long[] new_link_index_out, out long links_removed_out);
        [DllImport(Lib)] public static extern int rwr_graph_destroy(IntPtr g);
        [DllImport(Lib)] public static extern int rwr_graph_get_normalized(GraphHandle g, double[] w_out, byte[] dangling_out);
        [DllImport(Lib)] public static extern int rwr_get_stats(GraphHandle g, ref RwrStats stats_out);
        [DllImport(Lib)] public static extern int rwr_reset_stats(GraphHandle g);
        [DllImport(Lib)] public static extern int rwr_recommend(GraphHandle g, int seed, float d, int n_iter, int top_n,
            long[] out_id, double[] out_score, ref long inout_count);
        [DllImport(Lib)] public static extern int rwr_recommend_batch(GraphHandle g, int[] seeds, int K, float d, int n_iter,
            int top_n, long[] ids, double[] scores, int[] counts);
        // top_n (id, score) entries per seed among the nodes of type cand_type; the targets of the seed's raw links whose type has
        // its bit in excl_edge_mask are left out, and the seed itself when exclude_self != 0 (Recommender.RecommendationTypedBatch)
        [DllImport(Lib)] public static extern int rwr_recommend_typed_batch(GraphHandle g, int[] seeds, int K, float d, int n_iter,
            int top_n, int cand_type, uint excl_edge_mask, int exclude_self, long[] ids, double[] scores, int[] counts);
        // the audiences of K targets: list k ranks the nodes s of type cand_type (-1: any) by the score a walk FROM s gives
        // targets[k]; the sources of the raw links into targets[k] whose type has its bit in etype_mask are left out, and
        // targets[k] itself when exclude_self != 0; out_node may be null (Recommender.AudienceBatch)
        [DllImport(Lib)] public static extern int rwr_recommend_audience_batch(GraphHandle g, int K, int[] targets, float d, int n_iter, int cand_type, uint etype_mask, int exclude_self, int top_n, long[] out_id, double[] out_score, int[] out_node, int[] out_count);
        // the audiences of K weighted target sets (CSR: set_ptr, set_idx, set_w or null for 1.0 each), within an optional pool
        // of node indices (n_pool < 0: none) and with an optional deny list per set (Recommender.AudienceSetBatch)
        [DllImport(Lib)] public static extern int rwr_recommend_audience_set_batch(GraphHandle g, int K, long[] set_ptr, int[] set_idx, double[] set_w, float d, int n_iter, int cand_type, uint etype_mask, int exclude_members, int n_pool, int[] pool_idx, long[] deny_ptr, int[] deny_idx, int top_n, long[] out_id, double[] out_score, int[] out_node, int[] out_count);
        // ... with top_n up to 65 536: up to 1 024 entries the same lists, beyond them their continuation (Recommender.AudienceSetLongBatch)
        [DllImport(Lib)] public static extern int rwr_recommend_audience_set_long_batch(GraphHandle g, int K, long[] set_ptr, int[] set_idx, double[] set_w, float d, int n_iter, int cand_type, uint etype_mask, int exclude_members, int n_pool, int[] pool_idx, long[] deny_ptr, int[] deny_idx, int top_n, long[] out_id, double[] out_score, int[] out_node, int[] out_count);
        // ... and the position and score of every test id in those WHOLE lists (Recommender.AudienceSetPositionsBatch)
        [DllImport(Lib)] public static extern int rwr_recommend_audience_set_positions_batch(GraphHandle g, int K, long[] set_ptr, int[] set_idx, double[] set_w, float d, int n_iter, int cand_type, uint etype_mask, int exclude_members, int n_pool, int[] pool_idx, long[] deny_ptr, int[] deny_idx, long[] test_ptr, long[] test_ids, long[] out_pos, double[] out_score, long[] out_len);
        // the same K walks evaluated on the device: Hits and the running-precision sum (Experiment.cs:121-128) of every seed's WHOLE
        // list of type cand_type (its first top_n entries when top_n > 0, any value) against test set k; no list is written
        [DllImport(Lib)] public static extern int rwr_recommend_typed_eval_batch(GraphHandle g, int[] seeds, int K, float d, int n_iter,
            int top_n, int cand_type, uint excl_edge_mask, int exclude_self, long[] test_ptr, long[] test_ids, long[] n_hits,
            double[] sum_precision, long[] list_len);
        // ... and of every test entry its 0-based position and its score in the seed's WHOLE list of type cand_type (-1 / +0.0:
        // the list does not hold the id); pos_out and score_out are test_ptr[K] long, in the caller's order, list_len is K long
        [DllImport(Lib)] public static extern int rwr_recommend_typed_positions_batch(GraphHandle g, int[] seeds, int K, float d,
            int n_iter, int cand_type, uint excl_edge_mask, int exclude_self, long[] test_ptr, long[] test_ids, long[] pos_out,
            double[] score_out, long[] list_len);
        // the typed walks ranked within the caller's pool of node indices (pool_count < 0: no pool, pool_idx null; 0: an empty
        // pool) and with deny list k = deny_idx[deny_ptr[k] .. deny_ptr[k + 1]) never shown to seed k (deny_ptr null: none);
        // cand_type -1: nodes of any type (Recommender.RecommendationFilteredBatch)
        [DllImport(Lib)] public static extern int rwr_recommend_filtered_batch(GraphHandle g, int[] seeds, int K, float d, int n_iter,
            int top_n, int cand_type, uint excl_edge_mask, int exclude_self, long pool_count, int[] pool_idx, long[] deny_ptr,
            int[] deny_idx, long[] ids, double[] scores, int[] counts);
        // ... and the positions and scores of the test entries in the WHOLE filtered lists
        [DllImport(Lib)] public static extern int rwr_recommend_filtered_positions_batch(GraphHandle g, int[] seeds, int K, float d,
            int n_iter, int cand_type, uint excl_edge_mask, int exclude_self, long pool_count, int[] pool_idx, long[] deny_ptr,
            int[] deny_idx, long[] test_ptr, long[] test_ids, long[] pos_out, double[] score_out, long[] list_len);
        // the filtered walks with at most group_cap entries per group of nodes in every list: group_of = one label per node
        // (n values; < 0: never capped; null: no cap, group_cap ignored), group_cap in [1, 8] (Recommender.RecommendationCappedBatch)
        [DllImport(Lib)] public static extern int rwr_recommend_capped_batch(GraphHandle g, int[] seeds, int K, float d, int n_iter,
            int top_n, int cand_type, uint excl_edge_mask, int exclude_self, long pool_count, int[] pool_idx, long[] deny_ptr,
            int[] deny_idx, int[] group_of, int group_cap, long[] ids, double[] scores, int[] counts);
        // the capped lists with the reasons of every entry: nodes (K x top_n, may be null), why_src / why_term (K x top_n x n_why,
        // n_why in [0, 8]), why_total (K x top_n, may be null) (Recommender.RecommendationExplainedBatch)
        [DllImport(Lib)] public static extern int rwr_recommend_explained_batch(GraphHandle g, int[] seeds, int K, float d, int n_iter,
            int top_n, int cand_type, uint excl_edge_mask, int exclude_self, long pool_count, int[] pool_idx, long[] deny_ptr,
            int[] deny_idx, int[] group_of, int group_cap, int n_why, long[] ids, double[] scores, int[] counts, int[] nodes,
            int[] why_src, double[] why_term, long[] why_total);
        // the capped lists with top_n up to 65 536, ordered by score descending, id descending, node index ascending; nodes
        // (K x top_n, may be null) receives the entries' node indices (Recommender.RecommendationLongBatch)
        [DllImport(Lib)] public static extern int rwr_recommend_long_batch(GraphHandle g, int[] seeds, int K, float d, int n_iter, int top_n, int cand_type, uint excl_edge_mask, int exclude_self, long pool_count, int[] pool_idx, long[] deny_ptr, int[] deny_idx, int[] group_of, int group_cap, long[] ids, double[] scores, int[] counts, int[] nodes);
        // ... and the positions and scores of the test entries in the WHOLE capped lists
        [DllImport(Lib)] public static extern int rwr_recommend_capped_positions_batch(GraphHandle g, int[] seeds, int K, float d,
            int n_iter, int cand_type, uint excl_edge_mask, int exclude_self, long pool_count, int[] pool_idx, long[] deny_ptr,
            int[] deny_idx, int[] group_of, int group_cap, long[] test_ptr, long[] test_ids, long[] pos_out, double[] score_out,
            long[] list_len);
        // Hits / sum of precisions of Experiment.cs:121-128 computed on the device (the ranked list never crosses): one seed,
        // or K seeds with K test sets in CSR form (test set k = test_ids[test_ptr[k] .. test_ptr[k + 1]))
        [DllImport(Lib)] public static extern int rwr_recommend_eval(GraphHandle g, int seed, float d, int n_iter, long[] test_ids,
            long n_test, out long n_hits, out double sum_precision, out long list_len);
        [DllImport(Lib)] public static extern int rwr_recommend_eval_batch(GraphHandle g, int[] seeds, int K, float d, int n_iter,
            long[] test_ptr, long[] test_ids, long[] n_hits, double[] sum_precision, long[] list_len);
        // many ego-network-sized graphs at once: build + Recommendation(seed) + hits / sum of precisions per graph, a constant
        // number of launches for the whole batch (Recommender.EvaluateGraphs)
        [DllImport(Lib)] public static extern int rwr_eval_graphs(int count, RwrGraphDesc[] graphs, int[] seeds, float d, int n_iter,
            long[] test_ptr, long[] test_ids, ref RwrOpts opts, long[] n_hits, double[] sum_precision, long[] list_len);
        [DllImport(Lib)] public static extern int rwr_model_run(GraphHandle g, int seed, double d, int run_mode, double value,
            double[] rank_out, out long iters_out);

        [DllImport(Lib)] public static extern int rwr_model_deliver(GraphHandle g, int seed, double d, double[] rank, double[] next_rank);

        // K personalised Models in one call: rank_out is K x n row-major, iters_out K counts (Model.RunBatch)
        [DllImport(Lib)] public static extern int rwr_model_run_batch(GraphHandle g, int[] seeds, int K, double d, int run_mode,
            double value, double[] rank_out, long[] iters_out);

        [DllImport(Lib)] public static extern int rwr_model_run_restart_batch(GraphHandle g, int K, long[] sup_ptr, int[] sup_idx,
            double[] sup_val, int[] start, double d, int run_mode, double value, double[] rank_out, long[] iters_out);

        // the same K walks ranked on the device: top_n (id, score) entries per vector, the LIKEd items of the members of
        // exclusion set k (excl_ptr / excl_idx in CSR form; excl_ptr null: the nodes of vector k's support) left out
        [DllImport(Lib)] public static extern int rwr_recommend_restart_batch(GraphHandle g, int K, long[] sup_ptr, int[] sup_idx,
            double[] sup_val, int[] start, long[] excl_ptr, int[] excl_idx, double d, int n_iter, int top_n, long[] ids,
            double[] scores, int[] counts);

        // ... ranked among the nodes of type cand_type: the targets of the raw links whose type has its bit in excl_edge_mask of
        // every member of exclusion set k left out, and the members themselves when exclude_members != 0
        [DllImport(Lib)] public static extern int rwr_recommend_restart_typed_batch(GraphHandle g, int K, long[] sup_ptr, int[] sup_idx,
            double[] sup_val, int[] start, long[] excl_ptr, int[] excl_idx, double d, int n_iter, int top_n, int cand_type,
            uint excl_edge_mask, int exclude_members, long[] ids, double[] scores, int[] counts);

        // the same K walks evaluated on the device: Hits and the running-precision sum (Experiment.cs:121-128) of every vector's
        // list (its first top_n entries when top_n > 0) against test set k (test_ptr / test_ids in CSR form); no list is written
        [DllImport(Lib)] public static extern int rwr_recommend_restart_eval_batch(GraphHandle g, int K, long[] sup_ptr, int[] sup_idx,
            double[] sup_val, int[] start, long[] excl_ptr, int[] excl_idx, double d, int n_iter, int top_n, long[] test_ptr,
            long[] test_ids, long[] n_hits, double[] sum_precision, long[] list_len);

        // the positions and scores of the test entries in the WHOLE lists rwr_recommend_restart_typed_batch defines
        [DllImport(Lib)] public static extern int rwr_recommend_restart_typed_positions_batch(GraphHandle g, int K, long[] sup_ptr,
            int[] sup_idx, double[] sup_val, int[] start, long[] excl_ptr, int[] excl_idx, double d, int n_iter, int cand_type,
            uint excl_edge_mask, int exclude_members, long[] test_ptr, long[] test_ids, long[] pos_out, double[] score_out,
            long[] list_len);

        [DllImport(Lib)] public static extern int rwr_model_run_restart(GraphHandle g, double[] restart, double[] rank_in, double d,
            int run_mode, double value, double[] rank_out, out long iters_out);

        [DllImport(Lib)] public static extern int rwr_model_deliver_restart(GraphHandle g, double[] restart, double d, double[] rank,
            double[] next_rank);

        public static void Check(int status) {
            if (status == 0) return;
            string msg = Marshal.PtrToStringAnsi(rwr_last_error());
            switch (status) {
                case 2: throw new ArgumentOutOfRangeException(msg);            // RWR_E_RANGE
                case 1: throw new ArgumentException(msg);                      // RWR_E_INVALID
                case 5: throw new OutOfMemoryException(msg);                   // RWR_E_NOMEM
                case 7: throw new NotSupportedException(msg);                  // RWR_E_UNSUPPORTED
                default: throw new InvalidOperationException(msg);             // no device / HIP error
            }
        }
    }
}
