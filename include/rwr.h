/*
 * librwr -- MI355X-native Random-Walk-with-Restart engine, C-ABI boundary.
 *
 * This header is the drop-in boundary for the public surface of the reference's
 * namespace Recommenders.RWRBased (ChangUk/RecommenderSystems).  The reference is
 * 100 % managed C# with no FFI of its own; a thin C# shim (INTEGRATION.md,
 * csharp/Recommenders/RWRBased/) keeps the reference's public types and P/Invokes
 * exactly the entry points declared here.  Every entry point cites the reference
 * interface it replaces as file:line relative to the reference root.
 *
 * Conventions
 *   - plain C, plain pointers and sizes; no C++/torch types cross this boundary;
 *   - every function returns an int32 status (RWR_OK == 0); rwr_last_error() returns a
 *     thread-local UTF-8 message for the last failing call on the calling thread
 *     (the shim turns statuses into the .NET exceptions the reference would throw);
 *   - all pointers are HOST pointers unless a parameter says otherwise;
 *   - every entry point makes the graph's device current for the call and restores the calling
 *     thread's current HIP device before it returns;
 *   - handles are independent: distinct rwr_graph handles may be used concurrently from
 *     distinct host threads (the reference runs up to 10 worker threads, each with its
 *     own Graph/Recommender: Program.cs:11,61-66; Experiment.cs:71,104,108).  One handle
 *     must not be used from two threads at once;
 *   - there is NO CPU fallback: every compute entry point fails with RWR_E_NO_DEVICE
 *     when no gfx950 device is usable.
 */
#ifndef RWR_H
#define RWR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RWR_VERSION_STRING "0.4.0"

/* status codes */
enum {
    RWR_OK            = 0,
    RWR_E_INVALID     = 1,   /* bad argument (null pointer, negative size, malformed CSR)        */
    RWR_E_RANGE       = 2,   /* node index out of range  -> ArgumentOutOfRangeException/KeyNotFound */
    RWR_E_NO_DEVICE   = 3,   /* no usable HIP device                                             */
    RWR_E_HIP         = 4,   /* a HIP runtime call failed (message has the HIP error string)     */
    RWR_E_NOMEM       = 5,   /* host or device allocation failed                                 */
    RWR_E_CAPACITY    = 6,   /* caller's output buffer too small (needed size returned)          */
    RWR_E_UNSUPPORTED = 7    /* valid request this build does not implement                      */
};

/* enum NodeType { UNDEFINED, USER, ITEM, ETC }                     -- Recommender.cs:4 */
enum { RWR_NODE_UNDEFINED = 0, RWR_NODE_USER = 1, RWR_NODE_ITEM = 2, RWR_NODE_ETC = 3 };
/* enum EdgeType { UNDEFINED, LIKE, FRIENDSHIP, FOLLOW, MENTION, AUTHORSHIP, PURCHASE, ETC }
 *                                                                  -- Recommender.cs:5 */
enum { RWR_EDGE_UNDEFINED = 0, RWR_EDGE_LIKE = 1, RWR_EDGE_FRIENDSHIP = 2, RWR_EDGE_FOLLOW = 3,
       RWR_EDGE_MENTION = 4, RWR_EDGE_AUTHORSHIP = 5, RWR_EDGE_PURCHASE = 6, RWR_EDGE_ETC = 7 };

/* arithmetic mode of the power iteration.  There is one: every rank value is bitwise what
 * Model.deliverRanks (Model.cs:76-100) computes -- same addends, same order, no FMA contraction -- and
 * every ranked list is the reference's (Recommender.cs:35-38).  (Value 1 was RWR_MODE_FAST, a
 * re-associated mode without a ranking guarantee; it was removed in ABI 3 and rwr_graph_create
 * now rejects it with RWR_E_INVALID.) */
enum { RWR_MODE_EXACT = 0 };

/* rwr_model_run stop rule -- Model.run(int) / run(double) / run(): Model.cs:68-73,57-66,52-55 */
enum { RWR_RUN_ITERATIONS = 0, RWR_RUN_THRESHOLD = 1, RWR_RUN_DEFAULT_THRESHOLD = 2 };

typedef struct rwr_graph rwr_graph;   /* opaque: device-resident graph + workspaces + streams */

typedef struct rwr_opts {
    int32_t struct_size;     /* = sizeof(rwr_opts); lets the struct grow compatibly            */
    int32_t device;          /* HIP device ordinal; -1 = env RWR_DEVICE, else current device   */
    int32_t mode;            /* RWR_MODE_EXACT; -1 = default (EXACT)                           */
    int32_t tile_seeds;      /* seeds per rank-matrix tile (lanes per row): 1,2,4,8,16,32,64;
                                0 = auto                                                        */
    int32_t tile_group;      /* tiles iterated together (grid.y of the SpMM launch); 0 = auto  */
    int32_t profile;         /* 1 = bracket every kernel phase with HIP events (rwr_get_stats)  */
    int64_t workspace_bytes; /* cap on the batch workspace (rank matrices + sort buffers);
                                0 = auto (a fraction of free HBM)                               */
    int32_t seed_row_kernel; /* EXACT mode, how the seed's own row (the n-term restart chain,
                                Model.cs:91-93,96-97) is folded -- every choice is bitwise equal:
                                0 = auto (env RWR_CHAIN, else by batch size), 1 = sequential fold
                                beside the SpMM, 2 = parallel binade scan, 3 = simple one-lane loop */
    int32_t reserved0;
} rwr_opts;

/* accumulated since creation or the last rwr_reset_stats(); *_ms are device times measured
 * with HIP events on the library's own streams (only when opts.profile != 0) */
typedef struct rwr_stats {
    int32_t struct_size;
    int32_t n;               /* nodes                                                           */
    int64_t nnz_raw;         /* links handed over (incl. UNDEFINED)                             */
    int64_t nnz;             /* explicit links (type != UNDEFINED) = entries of P               */
    int32_t uniform;         /* 1 when every row's explicit raw weights are equal               */
    int32_t tile_seeds;      /* resolved seeds per tile of the last batch                       */
    int32_t tile_group;      /* resolved tiles per launch of the last batch                     */
    int32_t mode;
    double  build_ms;        /* device-side Graph.buildGraph + transpose (one-off)              */
    double  spmm_ms;         /* sum of SpMM launch durations                                    */
    int64_t spmm_launches;
    int64_t spmm_seed_steps; /* sum over launches of (seeds in the launch) -- one unit = one
                                power-iteration step of one seed                                */
    double  chain_ms;        /* seed-row kernels (sequential fold or binade scan)                */
    int64_t chain_launches;
    double  rank_ms;         /* exclusion mask + top-k / sort + gather (rwr_model_run_batch: the
                                extraction of finished columns into row-major staging)          */
    double  iterate_wall_ms; /* device time from the first to the last event of the iterate
                                phase (SpMM and seed-row kernels overlapped)                    */
    double  total_wall_ms;   /* host wall time inside rwr_recommend* calls                      */
    int64_t seeds_done;
    int64_t chain_redo_blocks; /* binade scan: blocks the carry had to redo row by row (binade
                                  crossings + mispredicted binades), summed over steps and seeds */
    /* the DENSE launches among spmm_launches: every row of the matrix is walked and every entry's
     * source row gathered (no frontier bitmap, no skipped rows).  Only these are priced with the full
     * algorithmic byte count by bench.py's roofline; the first iterations of a run, which skip the rows
     * that are still exactly zero, are not */
    double  spmm_dense_ms;
    int64_t spmm_dense_launches;
    int64_t spmm_dense_seed_steps;
    int32_t uniform_path;    /* 1 when the value-free matrix path serves this graph: every row's weights are
                                equal (unit raw weights, DataLoader.cs:293-294), so fl(fl((1-d) rank[i]) * weight)
                                (Model.cs:84,87) is ONE double per source node and step; the kernels gather it and
                                read no per-entry value (4 instead of 12 matrix bytes per entry) -- bitwise equal */
    int32_t reserved1;
    int64_t frontier_list_launches; /* SpMM launches of a batch's first steps that walked only each tile's
                                       frontier row list (the rows an out-link of a non-zero row reaches) */
    int64_t rank_fused_groups;      /* tile groups of rwr_recommend_batch whose ranking ran inside the last step: the
                                       step's second part kept only the rows that reach the seeds' thresholds */
    int64_t rank_fused_fallbacks;   /* ... groups that tried and ran the step whole after all: a seed's candidates
                                       did not fit its buffer */
    int64_t rank_pruned_rows;       /* ... (row, tile) pairs the second part skipped without gathering a rank row: the sum of
                                       a float bound over the row's in-list showed that no seed of the tile reaches its
                                       threshold there (groups that fell back count nothing); RWR_RANK_PRUNE=0: none */
    double  rank_bound_ms;          /* time of the bound tables and the rows' keep bits (part of rank_ms; profile only) */
    int64_t x_clear_skipped;        /* tile groups of rwr_recommend_batch that started without clearing their rank matrix: the
                                       fold beside step 2 read the frontier-list step's output through its bitmap (RWR_X_CLEAR=1:
                                       none) */
    int64_t entry_live_launches;    /* SpMM launches of rwr_recommend_batch's bitmap-probing steps that read the step's per-link
                                       tile masks instead of probing the frontier bitmaps per entry (RWR_ENTRY_LIVE=0: none) */
    /* which kernels served the single-seed SpMV steps (one rank vector: rwr_model_run / rwr_model_deliver and every
     * single-seed ranked call): launches of the source-block sweep, of the hub-row kernel (rows of >= RWR_HUB_T in-links)
     * and of the row-binned kernel.  Host-side counts; a step may launch all three */
    int64_t spmv_sweep_launches;
    int64_t spmv_hub_launches;
    int64_t spmv_binned_launches;
    /* the sweep's geometry as last decided for this graph (all 0 while undecided, after a rebuild, or when the graph does
     * not take the sweep; rwr_reset_stats leaves them, as it leaves n and uniform_path): slots of 64 rows per wave,
     * source blocks, workgroups, and 1 when the sweep serves the ITEM rows only (the other rows: the row-binned kernel) */
    int32_t sweep_k;
    int32_t sweep_blocks;
    int32_t sweep_wgs;
    int32_t sweep_partial;
} rwr_stats;

/* ---- library ------------------------------------------------------------------------- */

const char *rwr_version(void);
/* number of usable gfx950 devices (0 when none); never fails */
int32_t rwr_device_count(void);
/* message of the last failure on this thread ("" if none) */
const char *rwr_last_error(void);

/* ---- Graph ---------------------------------------------------------------------------
 * Replaces  new Graph(nodes, edges) + Graph.buildGraph()   (Graph.cs:45-49, 51-88; called
 * at Experiment.cs:104-105) and Graph.size() (Graph.cs:91-93).
 *
 * Input is the RAW link list exactly as the host built it, flattened in dictionary/list
 * order:  node i (0..n-1, the keys of Dictionary<int,Node>, Graph.cs:39) has
 * id node_id[i] / type node_type[i] (struct Node, Graph.cs:4-17) and out-links
 * rowptr[i]..rowptr[i+1]-1, each (dst, etype, w) = struct ForwardLink
 * {targetNode, type, weight} (Graph.cs:19-35) in List<ForwardLink> order
 * (Graph.cs:40).  Links are NOT filtered or normalised by the caller: the library drops
 * type == UNDEFINED links, sums the remaining weights of a source left to right and
 * divides (Graph.cs:57-81) on the device, then builds the in-neighbour (transposed) CSR
 * with entries ordered (source asc, list position asc) -- the addend order of
 * Model.deliverRanks.  A node without explicit links is dangling (Graph.cs:53,64,86).
 * A key missing from the edge dictionary is passed as an empty list.
 * The arrays are copied; the caller may free them after the call returns. */
int32_t rwr_graph_create(int32_t n, const int64_t *node_id, const uint8_t *node_type,
                         const int64_t *rowptr /* n+1 */, const int32_t *dst, const uint8_t *etype,
                         const double *w, const rwr_opts *opts /* may be NULL */, rwr_graph **out);
int32_t rwr_graph_destroy(rwr_graph *g);
/* Incremental rebuild.  The harness builds an almost identical graph for every fold and
 * methodology (new DataLoader + new Graph + buildGraph per fold, Experiment.cs:69-77,104-105),
 * and three methodologies differ from their base only by relabelling FRIENDSHIP links to
 * UNDEFINED (Experiment.cs:84-101).  When node list, rowptr and dst are unchanged, only the
 * links whose type or weight differ need to cross the boundary: link_index[q] is a position
 * in the flattened raw list given to rwr_graph_create (distinct positions), etype[q] / w[q]
 * its new type / raw weight (either array may be NULL = unchanged).  The library patches its
 * resident raw lists and re-runs Graph.buildGraph (Graph.cs:51-88) and the transpose on the
 * device; the resulting state is bit for bit what rwr_graph_create would build from the
 * patched lists.  count == 0 just rebuilds.  Not to be called concurrently with other calls
 * on the same handle.  Argument errors (RWR_E_INVALID / RWR_E_RANGE) are detected before
 * anything is patched and leave the graph as it was; a failure AFTER the patch (out of device
 * memory during the rebuild, a HIP error) invalidates the handle: every later call on it
 * fails with RWR_E_INVALID until it is destroyed.  Not in scope of THIS entry: links that join
 * or leave a list (rwr_graph_append_links, rwr_graph_remove_links, below; both move positions
 * handed out earlier, each by the formula in its comment). */
int32_t rwr_graph_update_links(rwr_graph *g, int64_t count, const int64_t *link_index,
                               const uint8_t *etype /* may be NULL */, const double *w /* may be NULL */);
/* Appends links to the resident graph: link q = (dst[q], etype[q], w[q]) goes to the END of node
 * src[q]'s list, which is what edges[src].Add(new ForwardLink(dst, etype, w)) does to the
 * reference's List<ForwardLink> (Graph.cs:40).  Links with the same src keep the order of q; src
 * need not be sorted.  The library merges them into its resident raw lists on the device (only
 * the new links cross the boundary) and re-runs Graph.buildGraph and the transpose there: the
 * resulting state -- normalised weights, dangling flags, in-neighbour lists, processing orders,
 * rwr_graph_size, the nnz_raw / nnz / uniform / uniform_path statistics -- is bit for bit what
 * rwr_graph_create would build from the patched lists, and every later call behaves accordingly
 * (a new LIKE link of a seed is excluded from its Recommendation, Recommender.cs:20-24).
 * etype values and weights are taken as rwr_graph_create takes them; a negative or NaN weight is
 * legal and moves the graph out of the Recommendation entries' domain (see rwr_recommend).
 * Positions: new_index_out[q] (may be NULL) is the position of link q in the NEW flattened raw
 * list, for a later rwr_graph_update_links.  Positions handed out earlier move: the link at old
 * position e of row i is now at e + (number of appended links with src < i).
 * count == 0 just rebuilds, as rwr_graph_update_links does.
 * Not in scope of THIS entry: appending NODES (rwr_graph_append_nodes, below, appends nodes and
 * links in one call) and REMOVING links (rwr_graph_remove_links, below, takes them out of their
 * lists; relabelling them to UNDEFINED through rwr_graph_update_links leaves the walk bit for bit
 * as if they were gone, but keeps them in the lists and in every count).
 * Errors, all found on the host before any device work; they leave the graph exactly as it was:
 * RWR_E_INVALID (g NULL, count < 0, a NULL src/dst/etype/w with count > 0, a handle invalidated
 * earlier), RWR_E_RANGE (a src[q] or dst[q] outside [0, n); the message names q),
 * RWR_E_UNSUPPORTED (nnz_raw + count beyond this build's limit of 2^32-2 links).
 * Failures come in two phases.  BEFORE THE SWAP: the merged lists are written into new buffers,
 * which the handle takes only when all of them exist; running out of device memory up to there
 * returns RWR_E_NOMEM and leaves the graph untouched and usable.  AFTER THE SWAP: a failure inside
 * the rebuild (out of device memory, a HIP error) invalidates the handle exactly as a failed
 * rwr_graph_update_links does: every later call on it fails with RWR_E_INVALID until it is
 * destroyed.  Not to be called concurrently with other calls on the same handle. */
int32_t rwr_graph_append_links(rwr_graph *g, int64_t count, const int32_t *src, const int32_t *dst,
                               const uint8_t *etype, const double *w,
                               int64_t *new_index_out /* count, may be NULL */);
/* Appends nodes behind the last node of the resident graph, and links in the same call.  New node
 * j gets index n + j, id node_id[j], type node_type[j] and an empty list, which is what
 * nodes.Add(n + j, new Node(id, type)); edges.Add(n + j, new List<ForwardLink>()) does to the
 * reference's dictionaries (Graph.cs:39-40).  The count links are then appended exactly as
 * rwr_graph_append_links appends them, with src[q] and dst[q] ranging over [0, n + n_new): a new
 * node may arrive with links to it and from it, and the call costs one rebuild.  Only the new
 * nodes and links cross the boundary.  The resulting state -- normalised weights, dangling flags,
 * in-neighbour lists, every processing order, both ITEM orders (equal ids rank in index order, as
 * rwr_graph_create ranks them), rwr_graph_size, the n / nnz_raw / nnz / uniform / uniform_path
 * statistics -- is bit for bit what rwr_graph_create would build from the grown arrays, and every
 * later call behaves accordingly: a personalised Model starts at rank[seed] = n + n_new
 * (Model.cs:44), so every score changes even when the new nodes have no links.  Node types are
 * taken as rwr_graph_create takes them (unchecked; anything but ITEM is no candidate).
 * n_new == 0 is rwr_graph_append_links, with identical results, positions and errors;
 * n_new > 0 with count == 0 is legal.  new_index_out as in rwr_graph_append_links.
 * A handle in row-partitioned use (rwr_part_begin was called) loses that state: the next
 * rwr_part_* call other than rwr_part_begin fails with RWR_E_INVALID.
 * Not in scope of THIS entry: REMOVING or renumbering nodes (rwr_graph_remove_nodes, below, takes
 * nodes out with their links and renumbers the others) and inserting a node anywhere but at the
 * end (create a new graph).  Links, of old and new nodes alike, leave through rwr_graph_remove_links.
 * Errors, all found on the host before any device work; they leave the graph exactly as it was:
 * RWR_E_INVALID (g NULL, n_new < 0, count < 0, a NULL node_id/node_type with n_new > 0, a NULL
 * src/dst/etype/w with count > 0, a handle invalidated earlier), RWR_E_RANGE (a src[q] or dst[q]
 * outside [0, n + n_new); the message names q and the new bound), RWR_E_UNSUPPORTED (n + n_new
 * beyond INT32_MAX; nnz_raw + count beyond this build's limit of 2^32-2 links).
 * Failures keep the two phases of rwr_graph_append_links: out of device memory before the swap
 * returns RWR_E_NOMEM and leaves the graph untouched and usable; a failure after the swap
 * invalidates the handle.  Not to be called concurrently with other calls on the same handle. */
int32_t rwr_graph_append_nodes(rwr_graph *g, int32_t n_new, const int64_t *node_id,
                               const uint8_t *node_type, int64_t count, const int32_t *src,
                               const int32_t *dst, const uint8_t *etype, const double *w,
                               int64_t *new_index_out /* count, may be NULL */);
/* Removes links from the resident graph: the links at the positions link_index[q] of the current
 * flattened raw list -- the currency of rwr_graph_update_links and of new_index_out -- leave their
 * lists, which is what edges[src].RemoveAt(k) does to the reference's List<ForwardLink>.  The
 * positions may come in any order; all must be distinct and lie in [0, nnz_raw).  Every surviving
 * link keeps its order within its list.  The library compacts its resident raw lists on the device
 * (only the positions cross the boundary) and re-runs Graph.buildGraph and the transpose there: the
 * resulting state -- normalised weights, dangling flags, in-neighbour lists, processing orders,
 * rwr_graph_size, the n / nnz_raw / nnz / uniform / uniform_path statistics -- is bit for bit what
 * rwr_graph_create would build from the shortened lists, and every later call behaves accordingly:
 * a removed LIKE link of a seed makes its target a candidate again (Recommender.cs:20-24), a
 * removed FOLLOW target reappears in the typed "who to follow" list, and a node that loses its
 * last explicit link becomes dangling.  Removing every link is legal and equals a create from
 * empty lists.  The memory of the removed links is given back (13 bytes each, plus 8 of the
 * normalised weight), and they no longer count against the limit of 2^32-2 links.
 * Positions handed out earlier move: the surviving link at old position e is now at
 * e - (number of removed positions < e).
 * count == 0 just rebuilds, as rwr_graph_update_links does.
 * A graph built in one launch (at most 8 192 nodes and 65 536 links) that grew past that size
 * does not return to the one-launch build when it shrinks again; its state is the same bits.
 * Errors, all found on the host before any device work; they leave the graph exactly as it was,
 * in this order: RWR_E_INVALID (g NULL; count < 0 or a NULL link_index with count > 0; a handle
 * invalidated earlier), RWR_E_RANGE (a position outside [0, nnz_raw); the message names the first
 * such q), RWR_E_INVALID (a position given twice; the message names the second occurrence's q).
 * Failures come in two phases.  BEFORE THE SWAP: the shortened lists are written into new buffers,
 * which the handle takes only when all of them exist; running out of device memory up to there
 * returns RWR_E_NOMEM and leaves the graph untouched and usable.  AFTER THE SWAP: a failure inside
 * the rebuild (out of device memory, a HIP error) invalidates the handle exactly as a failed
 * rwr_graph_update_links does: every later call on it fails with RWR_E_INVALID until it is
 * destroyed.  Not to be called concurrently with other calls on the same handle. */
int32_t rwr_graph_remove_links(rwr_graph *g, int64_t count, const int64_t *link_index);
/* Removes nodes from the resident graph: the nodes node_index[q] -- current node indices, in any
 * order, all distinct and inside [0, n) -- leave it, which is what nodes.Remove(i); edges.Remove(i)
 * plus a renumbering does to the reference's dictionaries.  Every raw link whose source OR target
 * is a removed node leaves with them; every other link keeps its order within its list.  The
 * surviving nodes close up and keep their order: old node i becomes
 * i - (number of removed nodes < i), and every surviving target is rewritten to the new index.
 * Only the node list crosses the boundary: the links that point TO a removed node are found on the
 * device, in the resident lists, which are compacted there together with the node arrays and both
 * ITEM orders.  Then Graph.buildGraph and the transpose are re-run there: the resulting state --
 * normalised weights, dangling flags, in-neighbour lists, processing orders, both ITEM orders
 * (equal ids rank in index order, as rwr_graph_create ranks them), rwr_graph_size,
 * rwr_graph_get_normalized, the n / nnz_raw / nnz / uniform / uniform_path statistics -- is bit for
 * bit what rwr_graph_create would build from the shortened and renumbered arrays, and every later
 * Model, Recommendation, typed, filtered, capped or explained call behaves accordingly: a removed
 * ITEM is in no list, a personalised Model starts at rank[seed] = n - count (Model.cs:44), and a
 * node whose every out-link pointed to removed nodes becomes dangling.
 * Outputs, each may be NULL, written only when the call succeeds (a refused call writes nothing):
 * new_node_index_out[i], i over the n nodes before the call, is the new index of old node i or -1
 * if it was removed; new_link_index_out[e], e over the nnz_raw positions before the call, is the
 * new position of that link in the flattened raw list -- the currency of rwr_graph_update_links
 * and rwr_graph_remove_links -- or -1; *links_removed_out is the number of links that left.
 * new_link_index_out is the one thing that makes a per-link array cross the boundary.
 * count == 0 just rebuilds, as rwr_graph_update_links does: both index outputs are the identity
 * and *links_removed_out is 0.
 * A handle in row-partitioned use (rwr_part_begin was called) loses that state, as in
 * rwr_graph_append_nodes.  The candidate lists of the typed entries are rebuilt by the next call
 * that needs them.  A graph built in one launch that grew past that size does not return to the
 * one-launch build when it shrinks again; its state is the same bits.
 * Errors, all found on the host before any device work; they leave the graph exactly as it was,
 * in this order: RWR_E_INVALID (g NULL; count < 0 or a NULL node_index with count > 0; a handle
 * invalidated earlier), RWR_E_RANGE (an index outside [0, n); the message names the first such q),
 * RWR_E_INVALID (an index given twice; the message names the second occurrence's q),
 * RWR_E_UNSUPPORTED (count == n: rwr_graph_create refuses n <= 0, so a graph cannot lose its last
 * node; destroy the graph instead).
 * Failures come in two phases.  BEFORE THE SWAP: everything is written into new buffers, which the
 * handle takes only when all of them exist and are filled; running out of device memory up to
 * there returns RWR_E_NOMEM and leaves the graph untouched and usable.  AFTER THE SWAP: a failure
 * inside the rebuild (out of device memory, a HIP error) invalidates the handle exactly as a failed
 * rwr_graph_update_links does: every later call on it fails with RWR_E_INVALID until it is
 * destroyed.  Not to be called concurrently with other calls on the same handle. */
int32_t rwr_graph_remove_nodes(rwr_graph *g, int32_t count, const int32_t *node_index,
                               int32_t *new_node_index_out /* n before the call, may be NULL */,
                               int64_t *new_link_index_out /* nnz_raw before the call, may be NULL */,
                               int64_t *links_removed_out /* may be NULL */);
/* Graph.size() (Graph.cs:91-93) plus link counts; any out pointer may be NULL */
int32_t rwr_graph_size(const rwr_graph *g, int32_t *n, int64_t *nnz_raw, int64_t *nnz_explicit);
/* Backs the public field Graph.graph (Graph.cs:43): w_out[e] = normalised weight of raw
 * link e (0 for UNDEFINED links, which the reference leaves out of graph[i]);
 * dangling_out[i] = 1 when graph[i] == null.  Either pointer may be NULL. */
int32_t rwr_graph_get_normalized(rwr_graph *g, double *w_out /* nnz_raw */, uint8_t *dangling_out /* n */);

/* ---- Recommender ---------------------------------------------------------------------
 * Replaces Recommender.Recommendation(int idxTargetUser, float dampingFactor, int nIteration)
 * (Recommender.cs:14-40) and the topN overload (Recommender.cs:42-51):
 *   personalised Model (Model.cs:33-50), run(nIteration) (Model.cs:68-73), exclusion of the
 *   seed's raw LIKE out-links (Recommender.cs:20-24), candidates = ITEM nodes not excluded
 *   (:27-31), sorted by score desc then id desc (:35-38).
 * d crosses as float and is widened natively, as Recommender.cs:16 -> Model.cs:33 does.
 * top_n <= 0 returns the whole list (the reference's Count == topN test never fires).
 * Domain: raw weights >= 0 with a positive finite sum per node (what the reference's loader
 * produces) and 0 <= d <= 1; on a graph with a negative / NaN weight or a zero row sum, or
 * for a damping factor outside [0, 1] (ranks would go negative), the Recommendation entries
 * fail with RWR_E_UNSUPPORTED (rwr_model_run still reproduces the reference there).
 * in:  *inout_count = capacity of out_id/out_score;  out: entries written.  If the list
 * needs more room the call fails with RWR_E_CAPACITY and *inout_count = required size
 * (n always suffices). */
int32_t rwr_recommend(rwr_graph *g, int32_t seed, float d, int32_t n_iter, int32_t top_n,
                      int64_t *out_id, double *out_score, int64_t *inout_count);

/* Recommendation + the evaluation the harness runs on its result (TweetRecommender/Experiment.cs:109,121-128):
 * walks the FULL ranked list and returns  n_hits = #{ranked ids in test_ids}  and
 * sum_precision = sum over hits, in rank order, of (double)hitsSoFar / (position + 1)  -- the harness then reports
 * n_hits and sum_precision / n_hits (Experiment.cs:131-138).  The list itself never leaves the device.
 * list_len (optional) receives the length of the ranked list. */
int32_t rwr_recommend_eval(rwr_graph *g, int32_t seed, float d, int32_t n_iter, const int64_t *test_ids,
                           int64_t n_test, int64_t *n_hits, double *sum_precision, int64_t *list_len);

/* The same for K seeds of one graph, each with its own test set: test set k = test_ids[test_ptr[k] .. test_ptr[k+1])
 * (CSR form, test_ptr has K + 1 entries).  n_hits / sum_precision / list_len (optional) have K entries; entry k is
 * exactly what rwr_recommend_eval(seeds[k], ..., test set k) returns.  The K full ranked lists are produced by the
 * batched iteration and evaluated where they lie (one workgroup per seed); nothing but 16 bytes per seed comes back. */
int32_t rwr_recommend_eval_batch(rwr_graph *g, const int32_t *seeds, int32_t K, float d, int32_t n_iter,
                                 const int64_t *test_ptr, const int64_t *test_ids, int64_t *n_hits,
                                 double *sum_precision, int64_t *list_len);

/* ---- Many small graphs at once ---------------------------------------------------------
 * The reference's own workload (TweetRecommender/Experiment.cs:64-134, ten threads of it: Program.cs:11) is thousands of
 * ego-network-sized graphs, each built once, asked ONE Recommendation(seed, d, nIteration) and evaluated against its fold's
 * test set.  Entry g of the batch is exactly
 *     rwr_graph_create(graphs[g]) ; rwr_recommend_eval(seeds[g], d, n_iter, test set g) ; rwr_graph_destroy
 * -- the same arrays, the same arithmetic, bit for bit -- but graphs that fit the one-launch build and the one-launch call
 * (up to 6144 nodes / 4096 items / 65536 links) share ONE build launch, ONE iteration launch and ONE evaluation launch for
 * the whole batch (a workgroup per graph) and three synchronisations in total; larger graphs of the batch take the calls
 * above one by one.  test set g = test_ids[test_ptr[g] .. test_ptr[g+1]); n_hits / sum_precision / list_len (optional)
 * have `count` entries.  opts as for rwr_graph_create (device, mode). */
typedef struct rwr_graph_desc {
    int32_t n_nodes;
    int32_t reserved0;
    const int64_t *node_id;        /* [n_nodes] */
    const uint8_t *node_type;      /* [n_nodes] */
    const int64_t *rowptr;         /* [n_nodes + 1] */
    const int32_t *dst;            /* [rowptr[n_nodes]] */
    const uint8_t *etype;
    const double *w;
} rwr_graph_desc;
int32_t rwr_eval_graphs(int32_t count, const rwr_graph_desc *graphs, const int32_t *seeds, float d, int32_t n_iter,
                        const int64_t *test_ptr, const int64_t *test_ids, const rwr_opts *opts, int64_t *n_hits,
                        double *sum_precision, int64_t *list_len);

/* Batch entry (an addition: the reference creates a fresh Model per call, Recommender.cs:16,
 * so seeds are independent and batching is semantically free).  top_n must be >= 1.
 * ids/scores are K x top_n row-major; counts[k] = entries valid in row k (the rest of the
 * row is id 0 / score 0).  Result k is exactly rwr_recommend(seeds[k], d, n_iter, top_n). */
int32_t rwr_recommend_batch(rwr_graph *g, const int32_t *seeds, int32_t K, float d, int32_t n_iter,
                            int32_t top_n, int64_t *ids, double *scores, int32_t *counts);
/* Recommendation among the nodes of ANY node type -- an addition beside the reference surface, whose Recommendation
 * (Recommender.cs:20-31) ranks ITEM nodes the seed does not LIKE and nothing else, while its loader links USER nodes by
 * FRIENDSHIP, FOLLOW and MENTION as well (DataLoader.cs:331-341, 359-360, 392): "who to follow" is candidates USER, mask
 * FRIENDSHIP | FOLLOW, exclude_self; "similar items" is candidates ITEM from an item seed, mask 0.
 * Result k: the rank row that rwr_model_run(g, seeds[k], (double)d, RWR_RUN_ITERATIONS, n_iter, ...) returns (d is widened
 * as Recommender.cs:16 widens it; a negative n_iter runs no step); of it
 *   - the candidates are the nodes with node_type == cand_type (any value 0..255: node types are unchecked at create);
 *   - a candidate is dropped when it is the target of a RAW out-link of the seed whose type t has bit (1u << t) set in
 *     excl_edge_mask (Recommender.cs:20-24 with the link type as a set; RWR_EDGE_UNDEFINED's bit is legal and drops the
 *     targets of UNDEFINED raw links), and the seed itself is dropped when exclude_self != 0;
 *   - the rest is ordered by score descending, then id descending (Recommender.cs:35-38); the first top_n of them go into
 *     row k of ids / scores (K x top_n, row-major), counts[k] = entries written, the rest of the row id 0 / score 0.
 * Ids are identical to that composition and scores bitwise equal to it, for every seed: duplicate seeds, dangling seeds and
 * seeds of another type than cand_type are allowed and give what the composition gives.
 *   - cand_type = RWR_NODE_ITEM, excl_edge_mask = 1u << RWR_EDGE_LIKE, exclude_self = 0 is rwr_recommend_batch: the same ids,
 *     scores and counts.
 *   - The domain is that of the Recommendation entries: a graph with a negative weight or d outside [0, 1] gives
 *     RWR_E_UNSUPPORTED (the ranking marks exclusions with -1 and relies on scores >= 0).
 *   - top_n in [1, 1024]: a larger top_n gives RWR_E_UNSUPPORTED with the limit in the message (whole lists of a node type
 *     are evaluated, not returned: rwr_recommend_typed_eval_batch).
 *   - Argument errors, all found before any device work: a NULL g is refused first; K == 0 is a no-op (RWR_OK); K < 0, NULL
 *     seeds / ids / scores / counts, top_n < 1, cand_type outside [0, 255] or a mask bit >= 8 give RWR_E_INVALID; a seed
 *     outside [0, n) gives RWR_E_RANGE with its batch position in the message.  A refused call writes nothing.
 *   - The candidate list of a node type is built on the device by the first call that names it and kept with the handle
 *     (four types at most; rwr_graph_append_nodes and rwr_graph_remove_nodes make the next call
 *     rebuild it).
 *   - opts.tile_seeds, tile_group and workspace_bytes keep their meaning (the seeds run as tiles of the batched SpMM). */
int32_t rwr_recommend_typed_batch(rwr_graph *g, const int32_t *seeds, int32_t K, float d, int32_t n_iter, int32_t top_n,
                                  int32_t cand_type, uint32_t excl_edge_mask, int32_t exclude_self,
                                  int64_t *ids, double *scores, int32_t *counts);
/* The same K walks evaluated on the device: Hits and the running-precision sum of every seed's list of one node type against
 * a test set (Experiment.cs:121-128), without the list ever being written -- "who to follow" scored against held-out FOLLOW
 * links.  seeds, d, n_iter, cand_type, excl_edge_mask, exclude_self and the domain exactly as in rwr_recommend_typed_batch.
 * Test set k is test_ids[test_ptr[k] .. test_ptr[k+1]) with HashSet<long> semantics, exactly as in
 * rwr_recommend_restart_eval_batch: duplicates change nothing, ids that no node carries are legal, a set may be empty.
 * Result k: let L_k be the WHOLE list rwr_recommend_typed_batch defines for seed k -- the same candidates, mask and self
 * exclusion, the same order, not cut at 1024 -- cut to its first top_n entries if top_n > 0 (any positive value, 1025
 * included) and kept whole if top_n <= 0.  n_hits[k] and sum_precision[k] are what Experiment.cs:121-128 computes over that
 * list -- hits numbered in rank order, the addends (double)nHits / (i + 1) summed in rank order -- and list_len[k] (may be
 * NULL) is the list's length.  The integers are equal to that composition and sum_precision bitwise equal to it, for every
 * seed: duplicate seeds, dangling seeds and seeds of another type than cand_type included.  Ids need not be unique among
 * nodes (rwr_graph_append_nodes): every candidate that carries a test id is a hit.
 *   - cand_type = RWR_NODE_ITEM, excl_edge_mask = 1u << RWR_EDGE_LIKE, exclude_self = 0, top_n <= 0 is
 *     rwr_recommend_eval_batch: the same integers, the same sums bit for bit.
 *   - A cand_type that no node carries gives n_hits 0, sum_precision +0.0, list_len 0 and RWR_OK.
 *   - Argument errors, all found before any device work and in this order: a NULL g is refused first; K == 0 is a no-op
 *     (RWR_OK); then everything rwr_recommend_typed_batch reports for K, the seeds, cand_type and the mask, with the same
 *     status and batch position (top_n has no bound here); then everything rwr_recommend_restart_eval_batch reports for
 *     test_ptr / test_ids / n_hits / sum_precision, with the same status and batch position; then the domain
 *     (RWR_E_UNSUPPORTED).  A refused call writes nothing.
 *   - The candidate list is the handle's cached one (rwr_recommend_typed_batch); opts.tile_seeds, tile_group and
 *     workspace_bytes keep their meaning. */
int32_t rwr_recommend_typed_eval_batch(rwr_graph *g, const int32_t *seeds, int32_t K, float d, int32_t n_iter, int32_t top_n,
                                       int32_t cand_type, uint32_t excl_edge_mask, int32_t exclude_self,
                                       const int64_t *test_ptr, const int64_t *test_ids,
                                       int64_t *n_hits, double *sum_precision, int64_t *list_len /* may be NULL */);
/* The same K walks, and of every test id its position and score in the seed's WHOLE list -- what MRR, NDCG@k, recall@k for
 * several k, AUC or "at which rank does item j appear for user u" are computed from on the host.  The counting of
 * rwr_recommend_typed_eval_batch knows every hit's position before it folds them into one sum; this entry returns them, and
 * still no list is written.  seeds, d, n_iter, cand_type, excl_edge_mask, exclude_self and the domain exactly as in
 * rwr_recommend_typed_batch; test_ptr / test_ids as in rwr_recommend_typed_eval_batch, but the entries are answered one by one.
 * Let L_k be the WHOLE list rwr_recommend_typed_batch defines for seed k -- the same candidates, mask and self exclusion, the
 * same order (score descending, then id descending, Recommender.cs:35-38), not cut anywhere: there is no top_n, the caller
 * cuts.  For every test entry j in [test_ptr[k], test_ptr[k+1]), in the caller's order and with duplicates kept:
 *   - pos_out[j] is the 0-based index in L_k of the FIRST entry whose id is test_ids[j], or -1 when L_k holds no such entry
 *     (no node carries the id, the node is of another type, or the candidate is excluded by the mask or as the seed itself);
 *   - score_out[j] (score_out may be NULL) is that entry's score, bitwise, and +0.0 when pos_out[j] == -1;
 *   - duplicate test entries receive the same answer; node ids need not be unique (rwr_graph_append_nodes): of several
 *     candidates carrying the id, the best-ranked one answers;
 *   - list_len[k] (list_len may be NULL) is the length of L_k.
 * The integers are identical, and the scores bitwise equal, to ranking the row that rwr_model_run(g, seeds[k], (double)d,
 * RWR_RUN_ITERATIONS, n_iter, ...) returns, for every seed: duplicate seeds (each with its own test entries), dangling seeds
 * and seeds of another type than cand_type included.  The result does not depend on scheduling: the same call gives the same
 * arrays.
 *   - cand_type = RWR_NODE_ITEM, excl_edge_mask = 1u << RWR_EDGE_LIKE, exclude_self = 0 gives the positions in rwr_recommend's
 *     whole list (top_n <= 0).
 *   - A cand_type that no node carries gives every pos_out -1, every score_out +0.0, list_len 0 and RWR_OK.
 *   - Argument errors, all found before any device work and in this order: a NULL g is refused first; K == 0 is a no-op
 *     (RWR_OK); then everything rwr_recommend_typed_batch reports for K, the seeds, cand_type and the mask, with the same
 *     status and batch position; then everything rwr_recommend_typed_eval_batch reports for test_ptr / test_ids, with pos_out
 *     in the place of its result arrays (a NULL pos_out with K > 0 gives RWR_E_INVALID); then the domain
 *     (RWR_E_UNSUPPORTED).  A refused call writes nothing.
 *   - test_ptr[K] x 16 bytes come back from the device; the candidate list is the handle's cached one
 *     (rwr_recommend_typed_batch); opts.tile_seeds, tile_group and workspace_bytes keep their meaning. */
int32_t rwr_recommend_typed_positions_batch(rwr_graph *g, const int32_t *seeds, int32_t K, float d, int32_t n_iter,
                                            int32_t cand_type, uint32_t excl_edge_mask, int32_t exclude_self,
                                            const int64_t *test_ptr, const int64_t *test_ids,
                                            int64_t *pos_out /* test_ptr[K] */, double *score_out /* test_ptr[K], may be NULL */,
                                            int64_t *list_len /* K, may be NULL */);
/* The typed walks ranked within a candidate pool the CALLER sets, and with a deny list per seed -- the two filters a serving
 * caller asks for first and that are not links of the graph: "rank only items published today / in stock / of one language"
 * (one pool for all seeds of the call, another one in the next call) and "never show seed k these nodes" (impressions already
 * served, blocked accounts, dismissed items).  Both are applied on the device, to the finished walk: the walk itself is that
 * of rwr_recommend_typed_batch, and so are seeds, d, n_iter, top_n, excl_edge_mask, exclude_self and the domain.
 * Result k starts from the rank row that rwr_model_run(g, seeds[k], (double)d, RWR_RUN_ITERATIONS, n_iter, ...) returns; of it
 *   - node i is a candidate when cand_type == -1 (nodes of ANY type) or node_type[i] == cand_type (0..255), AND pool_count < 0
 *     (no pool) or i occurs in pool_idx[0 .. pool_count).  The pool holds node INDICES, in any order, and may hold
 *     duplicates: a node listed twice is one candidate.  pool_count == 0 is an empty pool: every list is empty (counts 0) and
 *     the call returns RWR_OK;
 *   - a candidate is dropped when it is the target of a RAW out-link of the seed whose type has its bit in excl_edge_mask, or
 *     it is the seed and exclude_self != 0 (both exactly as in rwr_recommend_typed_batch), or it occurs in
 *     deny_idx[deny_ptr[k] .. deny_ptr[k+1]) (node indices; deny_ptr has K + 1 entries; deny_ptr == NULL: no deny lists).  A
 *     deny list may hold duplicates, the seed, nodes outside the pool and nodes of another type, and may be empty; duplicate
 *     seeds each keep their own deny list;
 *   - the rest is ordered by score descending, then id descending; the first top_n of them go into row k of ids / scores
 *     (K x top_n, row-major), counts[k] = entries written, the rest of the row id 0 / score 0.
 * Ids are identical to that composition and scores bitwise equal to it, for every seed; the same call gives the same arrays
 * twice (no atomic decides a position of the candidate list).
 *   - pool_count < 0, deny_ptr == NULL and cand_type >= 0 is rwr_recommend_typed_batch: the same ids, scores and counts.
 *   - top_n in [1, 1024]: a larger top_n gives RWR_E_UNSUPPORTED with the limit in the message, as the typed entry.
 *   - Argument errors, all found on the host before any device work and in this order: a NULL g is refused first; K == 0 is a
 *     no-op (RWR_OK); then everything rwr_recommend_typed_batch reports for K, the pointers, top_n < 1, cand_type (now
 *     [-1, 255]), the mask and the seeds, with the same status and batch position; pool_count > 0 with a NULL pool_idx
 *     (RWR_E_INVALID); a pool index outside [0, n) (RWR_E_RANGE, its position in the message); a deny_ptr that does not start
 *     at 0 or that decreases, a NULL deny_idx while deny_ptr[K] > 0 (RWR_E_INVALID); a deny index outside [0, n) (RWR_E_RANGE
 *     with its batch position); top_n's limit; the domain (RWR_E_UNSUPPORTED).  A refused call writes nothing.
 *   - The pool's candidate list is built on the device by every call that names a pool or cand_type -1 and dropped when the
 *     call ends: the handle's cached per-type lists (rwr_recommend_typed_batch) are neither read nor evicted by it, and a call
 *     without a pool and with cand_type >= 0 takes the cached list exactly as the typed entry does.
 *   - Not here: restart-vector walks; a Hits / AP destination of its own (the positions below give every metric); a pool per
 *     seed; pools given as node ids instead of indices (the host mirrors can map ids). */
int32_t rwr_recommend_filtered_batch(rwr_graph *g, const int32_t *seeds, int32_t K, float d, int32_t n_iter, int32_t top_n,
                                     int32_t cand_type, uint32_t excl_edge_mask, int32_t exclude_self,
                                     int64_t pool_count, const int32_t *pool_idx,
                                     const int64_t *deny_ptr /* K + 1, may be NULL */, const int32_t *deny_idx,
                                     int64_t *ids, double *scores, int32_t *counts);
/* ... and the positions and scores of test ids in the WHOLE filtered lists: rwr_recommend_typed_positions_batch over the lists
 * rwr_recommend_filtered_batch defines -- the same candidates (cand_type, the pool), the same exclusion (mask, self, deny
 * lists), the same order, not cut anywhere.  test_ptr, test_ids, pos_out, score_out (may be NULL) and list_len (may be NULL)
 * exactly as in rwr_recommend_typed_positions_batch: every test entry is answered in the caller's order, by the first list
 * entry carrying its id; a denied id, an id outside the pool and an id that no node carries answer -1 / +0.0; list_len[k] is
 * the length of the filtered list.  An empty pool gives every pos_out -1, every score_out +0.0, list_len 0 and RWR_OK.  The
 * integers are identical, and the scores bitwise equal, to ranking the row rwr_model_run returns.
 *   - pool_count < 0, deny_ptr == NULL and cand_type >= 0 is rwr_recommend_typed_positions_batch: the same arrays.
 *   - Argument errors, on the host before any device work and in this order: those of rwr_recommend_filtered_batch up to and
 *     including the deny lists (there is no top_n; the pointers are seeds); then everything
 *     rwr_recommend_typed_positions_batch reports for test_ptr / test_ids / pos_out; then the domain.  A refused call writes
 *     nothing.
 *   - Not here: what rwr_recommend_filtered_batch names. */
int32_t rwr_recommend_filtered_positions_batch(rwr_graph *g, const int32_t *seeds, int32_t K, float d, int32_t n_iter,
                                               int32_t cand_type, uint32_t excl_edge_mask, int32_t exclude_self,
                                               int64_t pool_count, const int32_t *pool_idx,
                                               const int64_t *deny_ptr /* K + 1, may be NULL */, const int32_t *deny_idx,
                                               const int64_t *test_ptr, const int64_t *test_ids,
                                               int64_t *pos_out /* test_ptr[K] */, double *score_out /* test_ptr[K], may be NULL */,
                                               int64_t *list_len /* K, may be NULL */);

/* The filtered walks with a diversity cap: at most group_cap entries per caller-set group of nodes in every seed's list -- "at
 * most 2 items per author", "at most 3 per category", "at most 1 per thread".  A group is neither a node type nor a link, and
 * over-fetching cannot stand in for it: one prolific author may fill every entry a call can return.  Everything but the two
 * new arguments is rwr_recommend_filtered_batch's, the walk, the domain and the layout of the result included.
 * group_of holds n int32 values, n the graph's current node count (appended nodes included): group_of[i] >= 0 is node i's
 * group label (any value, labels need not be dense), a negative value means "no group": that node is never capped.
 * Result k: let F_k be the WHOLE list rwr_recommend_filtered_batch defines for seed k -- the same candidates (cand_type, the
 * pool), the same exclusions (the link mask, self, the deny list), the same order (score descending, then id descending),
 * not cut anywhere.  F_k is walked from the top with a counter per label: an entry is kept when its label is negative or its
 * label's counter is below group_cap, and is then counted; otherwise it is dropped.  The kept entries are C_k; its first
 * top_n go into row k of ids / scores, counts[k] = entries written.  Ids are identical, and scores bitwise equal, to ranking
 * the row rwr_model_run returns; the same call gives the same arrays twice.
 *   - Candidates that the mask, self, the deny list or the pool remove do NOT use up a group's allowance: they are not in F_k,
 *     and the allowance goes to the group's next candidate.
 *   - The walk is "keep a candidate iff fewer than group_cap candidates of its label rank before it in F_k": a per-group,
 *     per-seed top-m, which is the form the device computes.
 *   - Two candidates of one group may be equal in score AND id (possible after rwr_graph_append_nodes; the rankers leave
 *     their mutual order unspecified): the cap keeps the one with the smaller node index.  The identity with the greedy walk
 *     is therefore promised only when (score, id) pairs are distinct within a group.
 *   - group_of == NULL (group_cap is ignored) is rwr_recommend_filtered_batch: the same arrays.  So is a group_cap of at
 *     least the largest group's size.  With pool_count < 0, deny_ptr == NULL and cand_type >= 0 as well it is
 *     rwr_recommend_typed_batch.
 *   - group_cap in [1, RWR_GROUP_CAP_MAX]: the selection keeps a column's best group_cap keys in registers.
 *   - Argument errors, all found on the host before any device work and in this order: everything
 *     rwr_recommend_filtered_batch reports up to and including the deny lists; group_of != NULL with group_cap < 1
 *     (RWR_E_INVALID); the limits -- top_n as there, then group_cap > RWR_GROUP_CAP_MAX (both RWR_E_UNSUPPORTED with the
 *     limit in the message); the domain.  A refused call writes nothing.
 *   - Not here: restart-vector walks; a Hits / AP destination of its own (the positions below give every metric); a cap per
 *     group or several labellings at once; labels kept with the handle. */
#define RWR_GROUP_CAP_MAX 8
int32_t rwr_recommend_capped_batch(rwr_graph *g, const int32_t *seeds, int32_t K, float d, int32_t n_iter, int32_t top_n,
                                   int32_t cand_type, uint32_t excl_edge_mask, int32_t exclude_self,
                                   int64_t pool_count, const int32_t *pool_idx,
                                   const int64_t *deny_ptr /* K + 1, may be NULL */, const int32_t *deny_idx,
                                   const int32_t *group_of /* n, may be NULL */, int32_t group_cap,
                                   int64_t *ids, double *scores, int32_t *counts);
/* ... and the positions and scores of test ids in the WHOLE capped lists C_k: rwr_recommend_filtered_positions_batch over the
 * lists rwr_recommend_capped_batch defines.  A candidate the cap drops answers -1 / +0.0, like a denied one; a kept one
 * answers its position in C_k; list_len[k] = |C_k|.
 *   - group_of == NULL is rwr_recommend_filtered_positions_batch: the same arrays.
 *   - Argument errors, on the host before any device work and in this order: those of rwr_recommend_filtered_positions_batch
 *     up to and including the test sets; group_of != NULL with group_cap < 1 (RWR_E_INVALID); group_cap >
 *     RWR_GROUP_CAP_MAX (RWR_E_UNSUPPORTED); the domain.  A refused call writes nothing.
 *   - Not here: what rwr_recommend_capped_batch names. */
int32_t rwr_recommend_capped_positions_batch(rwr_graph *g, const int32_t *seeds, int32_t K, float d, int32_t n_iter,
                                             int32_t cand_type, uint32_t excl_edge_mask, int32_t exclude_self,
                                             int64_t pool_count, const int32_t *pool_idx,
                                             const int64_t *deny_ptr /* K + 1, may be NULL */, const int32_t *deny_idx,
                                             const int32_t *group_of /* n, may be NULL */, int32_t group_cap,
                                             const int64_t *test_ptr, const int64_t *test_ids,
                                             int64_t *pos_out /* test_ptr[K] */, double *score_out /* test_ptr[K], may be NULL */,
                                             int64_t *list_len /* K, may be NULL */);

/* "Why is this entry here?" -- the capped lists with, per entry, its node index, its largest in-link addends and the number
 * of positive ones: "because users like you liked it", "liked by 37 users in your neighbourhood".  Everything up to group_cap
 * is rwr_recommend_capped_batch's: the walk, the domain, the candidates, every exclusion, the cap, the order and the layout of
 * ids / scores / counts, which are always bitwise those of the capped entry.  So the one entry also covers the filtered and
 * the typed lists (group_of == NULL, pool_count < 0, deny_ptr == NULL).
 *   - nodes[k * top_n + j] = the node index of list entry j of seed k (ids need not be unique, so the index cannot be
 *     recovered from the id).  Among candidates of one column with bitwise equal score and equal id the smaller node index
 *     ranks first -- the cap's choice -- which makes the order total: the same call gives the same arrays twice.  Cells at
 *     j >= counts[k] hold -1.
 *   - The in-list of an entry: let T = n_iter, v = nodes[k][j], y = the rank row rwr_model_run(g, seeds[k], (double)d,
 *     RWR_RUN_ITERATIONS, T - 1, ...) returns and c1 = 1 - (double)d.  The in-entries of v are the explicit links u -> v in
 *     the order source ascending, then list position ascending (the addend order of Model.deliverRanks).  Parallel links are
 *     separate entries; UNDEFINED links are not entries.  In-entry e has the addend a_e = fl(fl(c1 * y[u_e]) * w_e), w_e the
 *     normalised weight: two separately rounded products, no FMA.  For v other than the seed, scores[k][j] is the in-order
 *     sum of the a_e, bit for bit.
 *   - The reasons of (k, j) are the in-entries with a_e > 0, ordered by a_e descending, then in-list position ascending.  The
 *     first n_why of them go to why_src[(k * top_n + j) * n_why + .] (the source's node index) and why_term[...] (a_e,
 *     bitwise); unused cells hold -1 / +0.0.  why_total[k * top_n + j] = the number of in-entries with a_e > 0.
 *   - T <= 0: no step ran, so there are no reasons -- every why_total is 0 and every cell unused; the lists are still the
 *     capped entry's.
 *   - When v is the seed itself (exclude_self == 0 and a matching candidate type) the reasons cover its link addends only:
 *     the restart share of the seed's rank (Model.cs:91-97) is not a link and is not listed.
 *   - n_why in [0, RWR_WHY_MAX].  n_why == 0 ignores why_src and why_term, which may be NULL; nodes and why_total may be
 *     NULL.  With n_why == 0, nodes == NULL and why_total == NULL the entry is rwr_recommend_capped_batch, launch for launch.
 *   - Argument errors, all found on the host before any device work and in this order: everything
 *     rwr_recommend_capped_batch reports up to and including group_cap < 1; n_why < 0, or a NULL why_src / why_term with
 *     n_why > 0 (RWR_E_INVALID); the limits -- top_n, group_cap, then n_why > RWR_WHY_MAX (each RWR_E_UNSUPPORTED with the
 *     limit in the message); the domain.  A refused call writes nothing.
 *   - Not here: restart-vector walks; two-hop reasons ("because you liked A"); the edge type of a reason (the caller has
 *     why_src and its own lists); reasons for the evaluating and the positions destinations. */
#define RWR_WHY_MAX 8
int32_t rwr_recommend_explained_batch(rwr_graph *g, const int32_t *seeds, int32_t K, float d, int32_t n_iter, int32_t top_n,
                                      int32_t cand_type, uint32_t excl_edge_mask, int32_t exclude_self,
                                      int64_t pool_count, const int32_t *pool_idx,
                                      const int64_t *deny_ptr /* K + 1, may be NULL */, const int32_t *deny_idx,
                                      const int32_t *group_of /* n, may be NULL */, int32_t group_cap,
                                      int32_t n_why,
                                      int64_t *ids, double *scores, int32_t *counts,
                                      int32_t *nodes      /* K x top_n, may be NULL */,
                                      int32_t *why_src    /* K x top_n x n_why */,
                                      double  *why_term   /* K x top_n x n_why */,
                                      int64_t *why_total  /* K x top_n, may be NULL */);

/* The audience of an item -- an addition: the opposite question of every entry above.  Given K targets (nodes of any type;
 * they may repeat), list k ranks the nodes s of node type cand_type (-1: of any type) by
 *     S_k[s] ~ x_T^(s)[targets[k]],
 * the score a personalised walk of n_iter steps FROM s gives targets[k] -- "a tweet was just published, whom do we notify".
 * No walk from any s is run: the scores of all s at once are a reverse walk of n_iter steps from the target over the
 * out-link lists, with the restart mass of every s's walk (which depends on the dangling nodes it reaches) from one more
 * reverse walk of the dangling indicator.
 *   - Left out of list k: every s that has a raw link to targets[k] whose edge type has its bit in etype_mask (they already
 *     like or follow it; UNDEFINED links count when their bit is set, as in the typed entries), and with exclude_self
 *     targets[k] itself.  A bit of the mask beyond the edge types the header names is refused.
 *   - The order is score descending, then id descending, then node index ascending.  The tables are K x top_n; out_node
 *     (the entries' node indices, -1 behind a list's end) may be NULL; out_count[k] is the number of entries written.
 *   - Duality: s is in the whole audience list of v exactly when v is in the whole list of
 *     rwr_recommend_typed_batch(seed s, cand_type = the node type of v, the same mask, the same exclude_self).  The two
 *     scores agree to tol_rel (below).
 *   - Tolerance parity: this is the first ranking entry whose scores are NOT bitwise the forward walk's, because the addends
 *     of a sum arrive in another order.  All addends are >= 0, so no sum cancels; the one subtraction of the forward walk,
 *     rank - (1 - d) * rank, costs a factor 1 / d; a forward step sums at most n addends into a row, a reverse step at most
 *     the longest out-list.  Hence |S - x| <= tol_rel * x with
 *         tol_rel = 8 * (n_iter + 1) * (n + L + 8) * 2^-53 / d,   L = max(largest in-degree, largest out-degree),
 *     and where the forward score is +0.0 the reverse score is +0.0.  With d = 0 only S >= 0 and finiteness hold.
 *   - Determinism: the same call gives the same arrays twice, and list k does not depend on what else is in the batch or on
 *     K -- no floating-point atomics, a row's addends in list order.
 *   - Fixed n_iter >= 0 only: the threshold modes of Model.run have no reverse counterpart (a walk's own convergence test
 *     needs its own rank vector).  n_iter = 0 gives n at the target itself and 0 elsewhere.
 *   - Refusals, in this order: g NULL or a poisoned handle (RWR_E_INVALID); K < 0, or NULL targets, out_id, out_score or
 *     out_count with K > 0 (RWR_E_INVALID); a target outside [0, n) (RWR_E_RANGE, the message names k); top_n outside
 *     [1, 1024] (RWR_E_RANGE); n_iter < 0 (RWR_E_INVALID); cand_type outside [-1, 255] or a mask bit beyond the edge types
 *     (RWR_E_INVALID); the domain of the Recommendation entries -- a graph with a negative or non-finite normalised weight,
 *     or d outside [0, 1] (RWR_E_UNSUPPORTED); then K == 0 succeeds and touches nothing.  A refused call writes nothing.
 *   - Answered by rwr_recommend_audience_set_batch below: the duals of the restart-vector entries (weighted target sets), a
 *     pool of seeds and deny lists; Hits / average precision of audiences follow on the host from its positions entry.  Not
 *     here or there: a cap per group of seeds; negative weights. */
int32_t rwr_recommend_audience_batch(rwr_graph *g, int32_t K, const int32_t *targets, float d, int32_t n_iter,
                                     int32_t cand_type, uint32_t etype_mask, int32_t exclude_self, int32_t top_n,
                                     int64_t *out_id, double *out_score, int32_t *out_node /* K x top_n, may be NULL */,
                                     int32_t *out_count);

/* The audience of a weighted target SET -- an addition: a campaign, an author's items of today, a topic.  Set k is the
 * members set_idx[set_ptr[k] .. set_ptr[k + 1]) (node indices in [0, n), any order, any node type) with the weights set_w
 * beside them (> 0; set_w == NULL: every weight 1.0).  List k ranks the nodes s of cand_type (-1: of any type) by
 *     S_k[s] ~ sum over the distinct members v of set k of a_v * x_T^(s)[v],
 * x_T^(s) the rank row rwr_model_run(g, s, (double)d, RWR_RUN_ITERATIONS, n_iter, ...) returns: the dual of the
 * restart-vector walks.  The reverse walk is linear in its start and the restart mass does not depend on the target, so a
 * set costs the n_iter reverse steps of one target, started from sum_v a_v e_v.
 *   - A member that repeats in its set has its weights added on the host, in list order, before anything reaches the device
 *     (a_v above is that sum).  A node may belong to several sets, and a set may repeat in the batch.
 *   - Left out of list k: every s that has a raw link of a masked edge type to ANY member of set k (the mask test is
 *     rwr_recommend_audience_batch's); with exclude_members the members of set k themselves; the rows of deny list k
 *     (deny_idx[deny_ptr[k] .. deny_ptr[k + 1]), node indices; deny_ptr == NULL: none); and with n_pool >= 0 every node outside
 *     pool_idx[0 .. n_pool) -- node indices in any order, duplicates allowed, ONE pool for the whole call, intersected with
 *     cand_type as in rwr_recommend_filtered_batch; n_pool == 0 gives empty lists, n_pool < 0 means no pool.
 *   - The order, the K x top_n tables, out_node (may be NULL) and top_n in [1, 1024] are rwr_recommend_audience_batch's.
 *   - (a) One-member sets of weight 1.0 without pool and deny lists return bitwise what rwr_recommend_audience_batch returns
 *     for those targets -- ids, scores, nodes, counts -- with exclude_members in the place of exclude_self.
 *   - (b) Determinism: list k does not depend on K or on the rest of the batch, and the same call gives the same arrays
 *     twice -- no floating-point atomics.  A weight that is a power of two scales a one-member list's scores exactly.
 *   - (c) Scores do not depend on the pool or the deny lists: a narrowed list is bitwise the whole list with those rows
 *     struck out.
 *   - (d) Tolerance: |S - F| <= tol_rel * F for F = sum_v a_v x_T^(s)[v] summed in double, with
 *         tol_rel = 8 * (n_iter + 1) * (n + L + m + 8) * 2^-53 / d,   L as above, m = the largest set's size
 *     (a reverse step sums what it summed for one target; F adds m roundings of terms >= 0).  Where every forward addend is
 *     +0.0 the score is +0.0.
 *   - (e) Fixed n_iter >= 0 only, and the domain of rwr_recommend_audience_batch.  Weights are finite and in [2^-256, 2^256]:
 *     scores are <= n * (the sum of a set's weights), so none overflows.
 *   - Refusals, in this order: g NULL or a poisoned handle (RWR_E_INVALID); K < 0, or with K > 0 a NULL set_ptr, out_id,
 *     out_score or out_count (RWR_E_INVALID); the sets -- set_ptr[0] != 0, set_ptr decreasing, an empty set (the message
 *     names k), a NULL set_idx (all RWR_E_INVALID), then the first member outside [0, n) or weight that is not finite or
 *     outside [2^-256, 2^256] (RWR_E_RANGE, the message names k and the position in the set); top_n outside [1, 1024]
 *     (RWR_E_RANGE); n_iter < 0 (RWR_E_INVALID); cand_type outside [-1, 255] or a mask bit beyond the edge types
 *     (RWR_E_INVALID); n_pool > 0 with a NULL pool_idx (RWR_E_INVALID), a pool index outside [0, n) (RWR_E_RANGE); the deny
 *     lists as rwr_recommend_filtered_batch reports them; the domain (RWR_E_UNSUPPORTED); then K == 0 succeeds and touches
 *     nothing.  A refused call writes nothing.
 *   - Not here: a cache of the restart mass per handle; Hits / average precision as one device sum (the positions below give
 *     every metric on the host); a cap per group of seeds; negative weights. */
int32_t rwr_recommend_audience_set_batch(rwr_graph *g, int32_t K,
                                         const int64_t *set_ptr /* K + 1 */, const int32_t *set_idx,
                                         const double *set_w /* may be NULL: all 1.0 */,
                                         float d, int32_t n_iter, int32_t cand_type, uint32_t etype_mask, int32_t exclude_members,
                                         int32_t n_pool /* -1: no pool */, const int32_t *pool_idx,
                                         const int64_t *deny_ptr /* K + 1, may be NULL */, const int32_t *deny_idx,
                                         int32_t top_n, int64_t *out_id, double *out_score,
                                         int32_t *out_node /* K x top_n, may be NULL */, int32_t *out_count);
/* ... and the positions and scores of test ids in the WHOLE audience lists: rwr_recommend_filtered_positions_batch's
 * semantics over the lists rwr_recommend_audience_set_batch defines, not cut by any top_n.  For test id
 * test_ids[test_ptr[k] + j], out_pos holds the 0-based index of the first entry of list k with that id and out_score that
 * entry's score, bitwise the list's; an id the list does not hold (excluded, denied, outside the pool, of another type, carried
 * by no node) answers -1 / +0.0.  out_len[k] is the list's length.  A test id may repeat; a test set may be empty.
 *   - Refusals, in this order: those of rwr_recommend_audience_set_batch up to and including the deny lists, without the
 *     list tables and top_n; the test sets as rwr_recommend_filtered_positions_batch reports them (a NULL test_ptr or out_pos,
 *     test_ptr[0] != 0, test_ptr decreasing, a NULL test_ids: RWR_E_INVALID; a set of more than INT32_MAX ids:
 *     RWR_E_UNSUPPORTED); the domain; then K == 0 succeeds.  A refused call writes nothing. */
int32_t rwr_recommend_audience_set_positions_batch(rwr_graph *g, int32_t K,
                                                   const int64_t *set_ptr /* K + 1 */, const int32_t *set_idx,
                                                   const double *set_w /* may be NULL: all 1.0 */,
                                                   float d, int32_t n_iter, int32_t cand_type, uint32_t etype_mask,
                                                   int32_t exclude_members,
                                                   int32_t n_pool /* -1: no pool */, const int32_t *pool_idx,
                                                   const int64_t *deny_ptr /* K + 1, may be NULL */, const int32_t *deny_idx,
                                                   const int64_t *test_ptr /* K + 1 */, const int64_t *test_ids,
                                                   int64_t *out_pos /* test_ptr[K] */, double *out_score /* test_ptr[K], may be NULL */,
                                                   int64_t *out_len /* K, may be NULL */);

/* Ranked lists beyond 1 024 entries -- an addition: candidates for a re-ranker, a campaign's audience of 20 000 users.  The
 * two entries below take the argument lists of rwr_recommend_capped_batch and rwr_recommend_audience_set_batch with top_n in
 * [1, RWR_LONG_TOP_N_MAX]; no other entry changes its limit.
 *   - rwr_recommend_long_batch: list k is the rank row rwr_model_run(g, seeds[k], (double)d, RWR_RUN_ITERATIONS, n_iter, ...)
 *     returns, narrowed as rwr_recommend_capped_batch narrows it (cand_type, the masked links, exclude_self, the pool, deny
 *     list k, at most group_cap entries per group) and ranked by score descending, then id descending, then node index
 *     ascending -- a total order: ids and nodes are those of that ranking for any number of equal (score, id) pairs across
 *     the cut, scores are bitwise the row's, and the same call gives the same arrays twice.  The tables are K x top_n;
 *     nodes[k * top_n + j] is the node index of entry j (may be NULL); cells at j >= counts[k] hold 0 / +0.0 / -1.
 *   - top_n <= 1024 runs rwr_recommend_explained_batch with n_why == 0 and why_total == NULL, launch for launch, and returns
 *     that call's arrays.  Beyond, the lists are collected, sorted in runs of 4 096 entries and merged on the device; no
 *     floating-point atomic and no integer atomic's arrival order decides an entry.
 *   - Refusals of rwr_recommend_long_batch, in this order: everything rwr_recommend_capped_batch reports up to and including
 *     group_cap < 1 (RWR_E_INVALID / RWR_E_RANGE as there); the limits -- top_n > RWR_LONG_TOP_N_MAX, then group_cap >
 *     RWR_GROUP_CAP_MAX (both RWR_E_UNSUPPORTED with the limit in the message); the domain.  K == 0 succeeds after the graph
 *     and K are looked at, as there.  A refused call writes nothing.
 *   - rwr_recommend_audience_set_long_batch: rwr_recommend_audience_set_batch with top_n in [1, RWR_LONG_TOP_N_MAX] -- its
 *     sets, weights, exclusions, pool, deny lists, order, tolerance (d) and determinism (b), (c).  top_n <= 1024 returns that
 *     entry's arrays through the same body; a longer list continues it: its first 1 024 entries are bitwise that entry's
 *     list of top_n = 1024.  Refusals: that entry's, in its order, with top_n outside [1, RWR_LONG_TOP_N_MAX] (RWR_E_RANGE)
 *     in the place of its top_n step.
 *   - Memory: beside the K x top_n tables the device holds, per pass over some tiles of a tile group, two buffers of
 *     (top_n - 1 + 3072) entries of 24 bytes per list; a group whose buffers would pass 1 GiB is ranked tile by tile.  Running
 *     out of device memory is RWR_E_NOMEM.
 *   - Not here: long lists of the restart-vector walks; reasons (n_why > 0) for long lists; lists longer than
 *     RWR_LONG_TOP_N_MAX, which the positions entries answer; any change to rwr_recommend_batch's own sort path. */
#define RWR_LONG_TOP_N_MAX 65536
int32_t rwr_recommend_long_batch(rwr_graph *g, const int32_t *seeds, int32_t K, float d, int32_t n_iter, int32_t top_n,
                                 int32_t cand_type, uint32_t excl_edge_mask, int32_t exclude_self,
                                 int64_t pool_count, const int32_t *pool_idx,
                                 const int64_t *deny_ptr /* K + 1, may be NULL */, const int32_t *deny_idx,
                                 const int32_t *group_of /* n, may be NULL */, int32_t group_cap,
                                 int64_t *ids, double *scores, int32_t *counts,
                                 int32_t *nodes /* K x top_n, may be NULL */);
int32_t rwr_recommend_audience_set_long_batch(rwr_graph *g, int32_t K,
                                              const int64_t *set_ptr /* K + 1 */, const int32_t *set_idx,
                                              const double *set_w /* may be NULL: all 1.0 */,
                                              float d, int32_t n_iter, int32_t cand_type, uint32_t etype_mask, int32_t exclude_members,
                                              int32_t n_pool /* -1: no pool */, const int32_t *pool_idx,
                                              const int64_t *deny_ptr /* K + 1, may be NULL */, const int32_t *deny_idx,
                                              int32_t top_n, int64_t *out_id, double *out_score,
                                              int32_t *out_node /* K x top_n, may be NULL */, int32_t *out_count);

/* ---- Model ---------------------------------------------------------------------------
 * Backs the public class Model: ctor (Model.cs:33-50 personalised, seed >= 0;
 * Model.cs:14-31 global, seed == -1), run(int) / run(double) / run() (Model.cs:68-73,
 * 57-66, 52-55 incl. checkConvergence :110-115).  d is already a double here
 * (Model.cs:33 takes double).  rank_out receives Model.rank (n doubles) after the run;
 * iters_out (optional) the number of deliverRanks() calls made. */
int32_t rwr_model_run(rwr_graph *g, int32_t seed, double d, int32_t run_mode, double value,
                      double *rank_out, int64_t *iters_out);
/* K personalised Models (Model.cs:33-50) run in one call -- an addition beside the reference surface (every Model is
 * independent, Recommender.cs:16): row k of rank_out (K x n, row-major) and iters_out[k] are bitwise what
 * rwr_model_run(g, seeds[k], d, run_mode, value, ...) returns, for every run_mode, graph and damping factor that
 * rwr_model_run accepts (negative weights and d outside [0, 1] included: those run seed by seed).
 *   - Threshold modes: each seed stops at its own convergence step (the same diff < threshold test, Model.cs:58-65) and
 *     its row is the rank after that step.  A seed that does not converge within RWR_MAX_ITERS fails the whole call with
 *     RWR_E_UNSUPPORTED, as rwr_model_run does.
 *   - Argument errors, before any device work: K == 0 is a no-op (RWR_OK); K < 0, a NULL g, NULL seeds or NULL rank_out
 *     (K > 0) or an unknown run_mode give RWR_E_INVALID; a seed outside [0, n) -- -1 included: the global model stays on
 *     rwr_model_run -- gives RWR_E_RANGE with its batch position in the message.
 *   - Duplicate and dangling seeds are allowed.  iters_out may be NULL.
 *   - opts.tile_seeds, tile_group and workspace_bytes keep their meaning (the seeds run as tiles of the batched SpMM). */
int32_t rwr_model_run_batch(rwr_graph *g, const int32_t *seeds, int32_t K, double d, int32_t run_mode,
                            double value, double *rank_out, int64_t *iters_out);
/* ONE Model.deliverRanks() (Model.cs:76-100) on a rank vector held by the caller: next_rank = what the reference would
 * leave in nextRank (which updateRanks() has zeroed before, Model.cs:103-108) for the given rank.  Backs the public
 * step-by-step API -- deliverRanks / updateRanks / checkConvergence (Model.cs:76,103,110) -- for a host that drives the
 * loop itself; updateRanks and checkConvergence are array operations the shim does on its own copies.  seed >= 0:
 * personalised restart vector e_seed (bitwise in EXACT mode, for any rank vector); seed == -1: the global model's
 * uniform restart (tolerance parity, as rwr_model_run).  rank and next_rank hold n doubles and may not alias. */
int32_t rwr_model_deliver(rwr_graph *g, int32_t seed, double d, const double *rank, double *next_rank);

/* Model with a caller-set restart vector: the public field Model.restart (Model.cs:12), which deliverRanks reads on every
 * step (Model.cs:92-93 for rows with links, :96-97 for dangling rows) -- how a user of the reference runs multi-seed or
 * topic-weighted walks.  restart: n doubles, any finite values; rank_in: the starting rank (n doubles; may alias rank_out).
 * run_mode / value / rank_out / iters_out as rwr_model_run.  Bitwise in EXACT mode when at most RWR_RESTART_EXACT_MAX
 * entries of restart are non-zero (-0.0 counts as zero), tolerance parity otherwise (as the global model).  A NULL graph,
 * restart or rank pointer fails with RWR_E_INVALID; a non-finite entry of restart or of the rank with RWR_E_UNSUPPORTED
 * (inf * 0 would turn every row into NaN in the reference). */
#define RWR_RESTART_EXACT_MAX 256
int32_t rwr_model_run_restart(rwr_graph *g, const double *restart, const double *rank_in, double d,
                              int32_t run_mode, double value, double *rank_out, int64_t *iters_out);
/* ONE deliverRanks() with a caller-set restart vector (as rwr_model_deliver; rank and next_rank may alias) */
int32_t rwr_model_deliver_restart(rwr_graph *g, const double *restart, double d,
                                  const double *rank, double *next_rank);
/* K Models with caller-set restart vectors (Model.restart, Model.cs:12) run in one call -- an addition beside the reference
 * surface.  Vector k has the non-zero entries restart[sup_idx[q]] = sup_val[q], q in [sup_ptr[k], sup_ptr[k+1]), zero elsewhere.
 * start[k] >= 0: the personalised constructor's rank (Model.cs:44: n at start[k], 0 elsewhere); start[k] == -1: the global
 * constructor's (Model.cs:25: every rank 1).  start == NULL: all -1.
 * Row k of rank_out (K x n, row-major) and iters_out[k] are what
 *     rwr_model_run_restart(g, dense(v_k), rank0_k, d, run_mode, value, ...)
 * returns: bitwise whenever that call is bitwise (at most RWR_RESTART_EXACT_MAX non-zero entries), for every run_mode.
 *   - Argument errors, all found before any device work: a NULL g, K < 0, a NULL sup_ptr or rank_out, NULL sup_idx or
 *     sup_val while sup_ptr[K] > 0, a sup_ptr that does not start at 0 or that decreases, an unknown run_mode, or the same
 *     index twice within one vector (which a dense vector cannot express; the message carries k and the index) give
 *     RWR_E_INVALID; an index outside [0, n) or a start[k] outside [-1, n) gives RWR_E_RANGE with the batch position in the
 *     message; a non-finite sup_val gives RWR_E_UNSUPPORTED, as rwr_model_run_restart does.  K == 0 is a no-op (RWR_OK).
 *   - An entry whose value is +-0.0 is dropped (-0.0 counts as zero); an empty support is legal (a link-only walk).
 *   - Threshold modes: each vector stops at its own step (the reference's sequential |diff| sum, Model.cs:58-65, 110-115).
 *     A vector that does not converge within RWR_MAX_ITERS fails the whole call with RWR_E_UNSUPPORTED; the message names
 *     the smallest such k.  iters_out may be NULL.
 *   - A vector with more than RWR_RESTART_EXACT_MAX non-zero entries (the tolerance class), a graph with a negative
 *     weight, d outside [0, 1] or K == 1: the call runs vector by vector through rwr_model_run_restart, whose results it
 *     then returns.
 *   - opts.tile_seeds, tile_group and workspace_bytes keep their meaning (the vectors run as tiles of the batched SpMM). */
int32_t rwr_model_run_restart_batch(rwr_graph *g, int32_t K, const int64_t *sup_ptr, const int32_t *sup_idx,
                                    const double *sup_val, const int32_t *start, double d,
                                    int32_t run_mode, double value, double *rank_out, int64_t *iters_out);
/* The same K walks ranked on the device: the top_n candidates of every vector instead of its rank row -- the list a group
 * of users or a topic is recommended.  Vectors and starts exactly as in rwr_model_run_restart_batch; n_iter as Model.run(int)
 * (a negative count runs no step; there is no threshold mode: Recommendation takes an iteration count, Recommender.cs:14-18).
 * Exclusion set k is the node list excl_idx[excl_ptr[k] .. excl_ptr[k+1]): the RAW out-links of type LIKE of every node in it
 * are not candidates (Recommender.cs:20-24 applied to each member).  excl_ptr == NULL: set k is the indices listed in vector
 * k's support, whatever their values -- a group is not recommended what its members already like.  A node may appear twice
 * in a set; an empty set is legal; the support and start nodes themselves are NOT excluded (the reference does not exclude
 * the seed node either).
 * Result k: the rank row that rwr_model_run_restart(g, dense(v_k), rank0_k, d, RWR_RUN_ITERATIONS, n_iter, ...) returns; of
 * it the ITEM nodes that no member of set k LIKEs, by score descending, then id descending (Recommender.cs:35-38); the first
 * top_n of them in row k of ids / scores (K x top_n, row-major), counts[k] = entries written, the rest of the row id 0 /
 * score 0.  Ids are identical to that composition and scores bitwise equal to it, for every vector (K == 1 and a vector
 * with more than RWR_RESTART_EXACT_MAX non-zero entries run vector by vector through that very call).
 *   - The domain is that of the Recommendation entries: a graph with a negative weight, d outside [0, 1], a non-finite or a
 *     negative sup_val give RWR_E_UNSUPPORTED (the ranking marks exclusions with -1 and relies on scores >= 0;
 *     rwr_model_run_restart_batch remains the way to run signed vectors).
 *   - Argument errors, all found before any device work: everything rwr_model_run_restart_batch reports for the vectors,
 *     with the same status; NULL ids / scores / counts (K > 0), top_n < 1, an excl_ptr that does not start at 0 or that
 *     decreases, a NULL excl_idx while excl_ptr[K] > 0 give RWR_E_INVALID; an exclusion index outside [0, n) gives
 *     RWR_E_RANGE with the batch position in the message.  A NULL g is refused first; K == 0 is a no-op (RWR_OK).
 *     A refused call writes nothing. */
int32_t rwr_recommend_restart_batch(rwr_graph *g, int32_t K, const int64_t *sup_ptr, const int32_t *sup_idx,
                                    const double *sup_val, const int32_t *start, const int64_t *excl_ptr,
                                    const int32_t *excl_idx, double d, int32_t n_iter, int32_t top_n,
                                    int64_t *ids, double *scores, int32_t *counts);
/* The same K walks ranked among the nodes of ANY node type: "whom should this group follow".  Vectors, starts, n_iter, the
 * exclusion sets (excl_ptr == NULL: set k is the indices of vector k's support) and the domain exactly as in
 * rwr_recommend_restart_batch; cand_type and excl_edge_mask as in rwr_recommend_typed_batch.
 * Result k: the rank row that rwr_model_run_restart(g, dense(v_k), rank0_k, d, RWR_RUN_ITERATIONS, n_iter, ...) returns; of it
 *   - the candidates are the nodes with node_type == cand_type;
 *   - a candidate is dropped when it is the target of a RAW out-link of a member of set k whose type t has bit (1u << t) set
 *     in excl_edge_mask;
 *   - when exclude_members != 0 every member of set k is dropped as well (a group is not recommended its own members);
 *     start nodes are dropped only if they are members;
 *   - the rest is ordered by score descending, then id descending; the first top_n of them go into row k of ids / scores
 *     (K x top_n, row-major), counts[k] = entries written, the rest of the row id 0 / score 0.
 * Ids are identical to that composition and scores bitwise equal to it, for every vector (K == 1 and a vector with more than
 * RWR_RESTART_EXACT_MAX non-zero entries run vector by vector through that very call).  A node may appear twice in a set; an
 * empty set is legal; a member without raw links is still dropped by exclude_members.
 *   - cand_type = RWR_NODE_ITEM, excl_edge_mask = 1u << RWR_EDGE_LIKE, exclude_members = 0 is rwr_recommend_restart_batch: the
 *     same ids, scores and counts.
 *   - top_n in [1, 1024]: a larger top_n gives RWR_E_UNSUPPORTED with the limit in the message, as the typed seed entry.
 *   - Argument errors, all found before any device work: those of rwr_recommend_restart_batch, with the same status and batch
 *     position; cand_type outside [0, 255] or a mask bit >= 8 give RWR_E_INVALID.  A NULL g is refused first; K == 0 is a
 *     no-op (RWR_OK).  A refused call writes nothing. */
int32_t rwr_recommend_restart_typed_batch(rwr_graph *g, int32_t K, const int64_t *sup_ptr, const int32_t *sup_idx,
                                          const double *sup_val, const int32_t *start, const int64_t *excl_ptr,
                                          const int32_t *excl_idx, double d, int32_t n_iter, int32_t top_n,
                                          int32_t cand_type, uint32_t excl_edge_mask, int32_t exclude_members,
                                          int64_t *ids, double *scores, int32_t *counts);
/* The same K walks evaluated on the device: Hits and the running-precision sum of every vector's list against a test set
 * (Experiment.cs:121-128), without the list ever being written.  Vectors, starts, exclusion sets, d, n_iter and the domain
 * exactly as in rwr_recommend_restart_batch.  Test set k is test_ids[test_ptr[k] .. test_ptr[k+1]) with HashSet<long>
 * semantics: duplicates change nothing, ids that no node carries are legal, a set may be empty.
 * Result k: let L_k be the WHOLE list rwr_recommend_restart_batch defines for vector k (top_n = number of items), cut to its
 * first top_n entries if top_n > 0 (Hits@N / AP@N) and kept whole if top_n <= 0.  n_hits[k] and sum_precision[k] are what
 * Experiment.cs:121-128 computes over that list -- hits numbered in rank order, the addends (double)nHits / (i + 1) summed in
 * rank order -- and list_len[k] (may be NULL) is the list's length.  The integers are equal to that composition and
 * sum_precision bitwise equal to it, for every vector (the fallback classes of rwr_model_run_restart_batch included).
 * Item ids need not be unique (rwr_graph_append_nodes): every ITEM node that carries a test id is a hit.
 *   - Argument errors, all found before any device work: everything rwr_recommend_restart_batch reports for the vectors and
 *     the exclusion sets, with the same status and batch position; NULL test_ptr, n_hits or sum_precision (K > 0), a test_ptr
 *     that does not start at 0 or that decreases, a NULL test_ids while test_ptr[K] > 0 give RWR_E_INVALID; a set of more
 *     than INT32_MAX ids gives RWR_E_UNSUPPORTED.  A NULL g is refused first; K == 0 is a no-op (RWR_OK).  A refused call
 *     writes nothing. */
int32_t rwr_recommend_restart_eval_batch(rwr_graph *g, int32_t K, const int64_t *sup_ptr, const int32_t *sup_idx,
                                         const double *sup_val, const int32_t *start, const int64_t *excl_ptr,
                                         const int32_t *excl_idx, double d, int32_t n_iter, int32_t top_n,
                                         const int64_t *test_ptr, const int64_t *test_ids, int64_t *n_hits,
                                         double *sum_precision, int64_t *list_len /* may be NULL */);
/* The positions and scores of test ids in the WHOLE typed lists of K restart-vector walks: rwr_recommend_typed_positions_batch
 * for the walks of rwr_recommend_restart_typed_batch.  Vectors, starts, n_iter, the exclusion sets (excl_ptr == NULL: set k is
 * the indices of vector k's support), cand_type, excl_edge_mask, exclude_members and the domain exactly as in
 * rwr_recommend_restart_typed_batch; L_k is the whole list that entry defines for vector k, not cut anywhere (no top_n).
 * test_ptr, test_ids, pos_out, score_out (may be NULL) and list_len (may be NULL) exactly as in
 * rwr_recommend_typed_positions_batch: first entry carrying the id, -1 / +0.0 when there is none, duplicates answered alike,
 * the best-ranked of several candidates with one id.  The integers are identical, and the scores bitwise equal, to ranking
 * the row that rwr_model_run_restart(g, dense(v_k), rank0_k, d, RWR_RUN_ITERATIONS, n_iter, ...) returns, for every vector
 * (K == 1 and a vector with more than RWR_RESTART_EXACT_MAX non-zero entries run vector by vector through that very call).
 *   - A cand_type that no node carries gives every pos_out -1, every score_out +0.0, list_len 0 and RWR_OK.
 *   - Argument errors, all found before any device work and in this order: a NULL g is refused first; K == 0 is a no-op
 *     (RWR_OK); then K < 0 and a NULL sup_ptr (RWR_E_INVALID); cand_type outside [0, 255] or a mask bit >= 8
 *     (RWR_E_INVALID); everything rwr_recommend_restart_batch reports for the vectors and the exclusion sets, with the same
 *     status and batch position; everything rwr_recommend_restart_eval_batch reports for test_ptr / test_ids, with pos_out in
 *     the place of its result arrays (a NULL pos_out gives RWR_E_INVALID); then the domain (RWR_E_UNSUPPORTED).  A refused
 *     call writes nothing. */
int32_t rwr_recommend_restart_typed_positions_batch(rwr_graph *g, int32_t K, const int64_t *sup_ptr, const int32_t *sup_idx,
                                                    const double *sup_val, const int32_t *start, const int64_t *excl_ptr,
                                                    const int32_t *excl_idx, double d, int32_t n_iter, int32_t cand_type,
                                                    uint32_t excl_edge_mask, int32_t exclude_members,
                                                    const int64_t *test_ptr, const int64_t *test_ids, int64_t *pos_out,
                                                    double *score_out /* may be NULL */, int64_t *list_len /* may be NULL */);

/* ---- row-partitioned mode (graphs beyond one GPU; BASELINE.json config 5) ------------
 * An ADDITION: the reference has no distributed mode.  The transition matrix is partitioned by SOURCE rows
 * (the reference's native layout: graph[i] = out-links of i, Graph.cs:43): rank r owns the contiguous node slab
 * [slab_lo, slab_hi) and creates its rwr_graph from the FULL node arrays but with out-links only for its own
 * rows (rowptr flat outside the slab).  Every rank keeps the full rank matrix x[n][G] (G = tile width,
 * K <= 64 seeds); one power-iteration step is
 *     rwr_part_local_step    y = (1-d) * P_slab^T x   over ALL n rows,  r[k] = restart mass of the slab's rows
 *     (caller)               all-reduce(sum) of y and r over the ranks  -- RCCL over xGMI, torch.distributed
 *     rwr_part_finish_step   y[seed_k][k] += r[k]      (Model.cs:91-93,96-97)
 * after which y is the next x.  dev_* are DEVICE pointers owned by the caller (n*G, n*G and G doubles).
 * A rank's link-only partial y IS bitwise, for any x and whichever step of the walk it is: every row the list-order
 * sum, from 0.0, of the addends fl(fl((1-d) x[i][k]) * w) of its in-links from the slab (source ascending, list
 * position ascending; no FMA) -- the arithmetic of the batch path; rows no in-slab source reaches and the padding
 * columns are +0.0, and only the slab's rows of x are read.  What re-associates is the restart mass r (a tree sum
 * over the slab's rows) and the sum over the ranks: parity of the WALK with the single-GPU result is therefore to
 * tolerance (scores within 1e-6; identical top-k lists in the tests).  rwr_part_rank ranks the seeds whose row
 * this rank owns (only the owner holds the seed's raw LIKE links for the exclusion list,
 * Recommender.cs:20-24) and reports counts[k] = -1 for the others. */
int32_t rwr_part_begin(rwr_graph *g, int32_t slab_lo, int32_t slab_hi, const int32_t *seeds, int32_t K, double d,
                       void *dev_x, int32_t *tile_seeds_out);
/* The preferred step: ONE asynchronous call per iteration, enqueued on the CALLER's HIP stream (`stream` = a hipStream_t,
 * e.g. the stream torch.distributed / RCCL is ordered after; NULL = the device's default stream, which is what
 * torch.cuda.current_stream() denotes unless the caller switched streams) with no host synchronisation:
 *     y = (1-d) * P_slab^T x  over ALL n rows,  then  y[seed_k][k] += restart mass of the slab's rows  (Model.cs:91-93,96-97)
 * so that the sum over the ranks of y is the complete next rank matrix.  A rank only ever READS its own slab of x (its
 * graph holds out-links of its own rows only), so the exchange is a REDUCE-SCATTER of y by slabs -- half the bytes of an
 * all-reduce, and no second collective for the restart scalars; only the last step needs every row everywhere (ranking)
 * and uses an all-reduce.  recommendersystems_amd/partitioned.py is the host logic. */
int32_t rwr_part_step(rwr_graph *g, const void *dev_x, void *dev_y, void *stream);
int32_t rwr_part_local_step(rwr_graph *g, const void *dev_x, void *dev_y, void *dev_r);
int32_t rwr_part_finish_step(rwr_graph *g, void *dev_y, const void *dev_r);
int32_t rwr_part_rank(rwr_graph *g, void *dev_x, int32_t top_n, int64_t *ids, double *scores, int32_t *counts);

/* ---- measurement ---------------------------------------------------------------------- */
int32_t rwr_get_stats(rwr_graph *g, rwr_stats *out);
int32_t rwr_reset_stats(rwr_graph *g);

#ifdef __cplusplus
}
#endif
#endif /* RWR_H */
