// Drop-in replacement of Recommenders/RWRBased/Recommender.cs: same enums (same member order = same integer
// values, they cross the C-ABI as bytes) and the same two Recommendation overloads.
using System.Collections.Generic;

namespace Recommenders.RWRBased {
    public enum NodeType { UNDEFINED, USER, ITEM, ETC }
    public enum EdgeType { UNDEFINED, LIKE, FRIENDSHIP, FOLLOW, MENTION, AUTHORSHIP, PURCHASE, ETC }

    public class Recommender {
        private Graph graph;
        public Recommender(Graph graph) { this.graph = graph; }

        public List<KeyValuePair<long, double>> Recommendation(int idxTargetUser, float dampingFactor, int nIteration) {
            return Recommendation(idxTargetUser, dampingFactor, nIteration, 0);
        }

        public List<KeyValuePair<long, double>> Recommendation(int idxTargetUser, float dampingFactor, int nIteration, int topN) {
            // the reference reads graph.edges[idxTargetUser] and throws KeyNotFoundException when absent
            if (!graph.edges.ContainsKey(idxTargetUser)) throw new KeyNotFoundException();
            long count = graph.size();
            var ids = new long[count]; var scores = new double[count];
            Native.Check(Native.rwr_recommend(graph.handle, idxTargetUser, dampingFactor, nIteration, topN, ids, scores, ref count));
            var result = new List<KeyValuePair<long, double>>((int)count);
            for (long i = 0; i < count; i++) result.Add(new KeyValuePair<long, double>(ids[i], scores[i]));
            return result;
        }

        // addition: the harness's loop body (Experiment.cs:69-134) for MANY graphs in one call -- graphs[k].buildGraph(),
        // Recommendation(seeds[k], d, nIteration) and the hits / sum-of-precisions walk over testSets[k] -- without building the
        // Graph objects one by one.  hits[k] and sumPrecision[k] are exactly what the loop computes for graph k.
        public static void EvaluateGraphs(Graph[] graphs, int[] seeds, float dampingFactor, int nIteration, HashSet<long>[] testSets,
                                          out long[] hits, out double[] sumPrecision) {
            int K = graphs.Length;
            var descs = new RwrGraphDesc[K];
            var pins = new List<System.Runtime.InteropServices.GCHandle>();
            System.Func<object, System.IntPtr> pin = a => {
                var h = System.Runtime.InteropServices.GCHandle.Alloc(a, System.Runtime.InteropServices.GCHandleType.Pinned);
                pins.Add(h);
                return h.AddrOfPinnedObject();
            };
            var testPtr = new long[K + 1];
            var testIds = new List<long>();
            try {
                for (int k = 0; k < K; k++) {
                    long[] nodeId; byte[] nodeType; long[] rowptr; int[] dst; byte[] etype; double[] w;
                    graphs[k].Flatten(out nodeId, out nodeType, out rowptr, out dst, out etype, out w);
                    descs[k] = new RwrGraphDesc { n_nodes = nodeId.Length, reserved0 = 0, node_id = pin(nodeId), node_type = pin(nodeType),
                                                  rowptr = pin(rowptr), dst = pin(dst), etype = pin(etype), w = pin(w) };
                    testIds.AddRange(testSets[k]);
                    testPtr[k + 1] = testIds.Count;
                }
                hits = new long[K]; sumPrecision = new double[K];
                var opts = new RwrOpts { struct_size = System.Runtime.InteropServices.Marshal.SizeOf(typeof(RwrOpts)), device = -1, mode = -1 };
                Native.Check(Native.rwr_eval_graphs(K, descs, seeds, dampingFactor, nIteration, testPtr, testIds.ToArray(), ref opts, hits,
                                                    sumPrecision, null));
            } finally {
                foreach (var h in pins) h.Free();
            }
        }

        // addition: many seeds in one call (results identical to calling Recommendation per seed)
        public List<KeyValuePair<long, double>>[] RecommendationBatch(int[] seeds, float dampingFactor, int nIteration, int topN) {
            if (topN < 1) throw new System.ArgumentOutOfRangeException("topN", "RecommendationBatch needs topN >= 1 (rwr_recommend_batch)");
            int K = seeds.Length;
            var ids = new long[(long)K * topN]; var scores = new double[(long)K * topN]; var counts = new int[K];
            Native.Check(Native.rwr_recommend_batch(graph.handle, seeds, K, dampingFactor, nIteration, topN, ids, scores, counts));
            var all = new List<KeyValuePair<long, double>>[K];
            for (int k = 0; k < K; k++) {
                all[k] = new List<KeyValuePair<long, double>>(counts[k]);
                for (int q = 0; q < counts[k]; q++) all[k].Add(new KeyValuePair<long, double>(ids[(long)k * topN + q], scores[(long)k * topN + q]));
            }
            return all;
        }

        // addition: the audiences of K targets (rwr_recommend_audience_batch) -- list k ranks the nodes s of candType (null: of
        // any type) by the score a walk of nIteration steps FROM s gives targets[k], by one reverse walk per target.  The nodes
        // with a raw link of a type in exclEdgeTypes to targets[k] are left out, targets[k] itself too with excludeSelf.  The
        // scores agree with the forward walks' to the tolerance rwr.h derives, not bitwise
        public List<KeyValuePair<long, double>>[] AudienceBatch(int[] targets, float dampingFactor, int nIteration, NodeType? candType = null,
                                                                IEnumerable<EdgeType> exclEdgeTypes = null, bool excludeSelf = false,
                                                                int topN = 100) {
            if (topN < 1) throw new System.ArgumentOutOfRangeException("topN", "AudienceBatch needs topN >= 1");
            int K = targets.Length;
            uint mask = 0;
            if (exclEdgeTypes != null) foreach (var t in exclEdgeTypes) mask |= 1u << (int)t;
            var ids = new long[(long)K * topN]; var scores = new double[(long)K * topN]; var counts = new int[K];
            Native.Check(Native.rwr_recommend_audience_batch(graph.handle, K, targets, dampingFactor, nIteration, candType.HasValue ? (int)candType.Value : -1, mask, excludeSelf ? 1 : 0, topN, ids, scores, null, counts));
            var all = new List<KeyValuePair<long, double>>[K];
            for (int k = 0; k < K; k++) {
                all[k] = new List<KeyValuePair<long, double>>(counts[k]);
                for (int q = 0; q < counts[k]; q++) all[k].Add(new KeyValuePair<long, double>(ids[(long)k * topN + q], scores[(long)k * topN + q]));
            }
            return all;
        }

        // ... and for one target
        public List<KeyValuePair<long, double>> Audience(int target, float dampingFactor, int nIteration, NodeType? candType = null,
                                                         IEnumerable<EdgeType> exclEdgeTypes = null, bool excludeSelf = false, int topN = 100) {
            return AudienceBatch(new[] { target }, dampingFactor, nIteration, candType, exclEdgeTypes, excludeSelf, topN)[0];
        }

        // addition: the audiences of K weighted target sets (rwr_recommend_audience_set_batch) -- list k ranks the nodes s of
        // candType (null: any type) by the weighted sum of the scores a walk FROM s gives the members of sets[k].  weights:
        // null for 1.0 each, else one weight per member (a member that repeats has its weights added).  Left out: the nodes
        // with a raw link of a type in exclEdgeTypes to any member, the members with excludeMembers, the node indices of
        // deny[k] (deny null: none), and with a pool (node indices, any order) every node outside it
        public List<KeyValuePair<long, double>>[] AudienceSetBatch(int[][] sets, float dampingFactor, int nIteration, double[][] weights = null,
                                                                   NodeType? candType = null, IEnumerable<EdgeType> exclEdgeTypes = null,
                                                                   bool excludeMembers = false, int[] pool = null, int[][] deny = null,
                                                                   int topN = 100) {
            if (topN < 1) throw new System.ArgumentOutOfRangeException("topN", "AudienceSetBatch needs topN >= 1");
            int K = sets.Length;
            long[] setPtr, denyPtr; int[] setIdx, denyIdx; double[] setW; uint mask;
            PackAudienceSets(sets, weights, exclEdgeTypes, deny, out setPtr, out setIdx, out setW, out denyPtr, out denyIdx, out mask);
            var ids = new long[(long)K * topN]; var scores = new double[(long)K * topN]; var counts = new int[K];
            Native.Check(Native.rwr_recommend_audience_set_batch(graph.handle, K, setPtr, setIdx, setW, dampingFactor, nIteration, candType.HasValue ? (int)candType.Value : -1, mask, excludeMembers ? 1 : 0, pool == null ? -1 : pool.Length, pool == null || pool.Length == 0 ? new int[1] : pool, denyPtr, denyIdx, topN, ids, scores, null, counts));
            var all = new List<KeyValuePair<long, double>>[K];
            for (int k = 0; k < K; k++) {
                all[k] = new List<KeyValuePair<long, double>>(counts[k]);
                for (int q = 0; q < counts[k]; q++) all[k].Add(new KeyValuePair<long, double>(ids[(long)k * topN + q], scores[(long)k * topN + q]));
            }
            return all;
        }

        // ... for one set
        public List<KeyValuePair<long, double>> AudienceSet(int[] members, float dampingFactor, int nIteration, double[] weights = null,
                                                            NodeType? candType = null, IEnumerable<EdgeType> exclEdgeTypes = null,
                                                            bool excludeMembers = false, int[] pool = null, int[] deny = null, int topN = 100) {
            return AudienceSetBatch(new[] { members }, dampingFactor, nIteration, weights == null ? null : new[] { weights }, candType,
                                    exclEdgeTypes, excludeMembers, pool, deny == null ? null : new[] { deny }, topN)[0];
        }

        // addition: AudienceSetBatch for lists of up to 65 536 entries (rwr_recommend_audience_set_long_batch): up to 1 024 entries
        // it returns AudienceSetBatch's lists, a longer list continues them
        public List<KeyValuePair<long, double>>[] AudienceSetLongBatch(int[][] sets, float dampingFactor, int nIteration, double[][] weights = null,
                                                                       NodeType? candType = null, IEnumerable<EdgeType> exclEdgeTypes = null,
                                                                       bool excludeMembers = false, int[] pool = null, int[][] deny = null,
                                                                       int topN = 4096) {
            if (topN < 1) throw new System.ArgumentOutOfRangeException("topN", "AudienceSetLongBatch needs topN >= 1");
            int K = sets.Length;
            long[] setPtr, denyPtr; int[] setIdx, denyIdx; double[] setW; uint mask;
            PackAudienceSets(sets, weights, exclEdgeTypes, deny, out setPtr, out setIdx, out setW, out denyPtr, out denyIdx, out mask);
            var ids = new long[(long)K * topN]; var scores = new double[(long)K * topN]; var counts = new int[K];
            Native.Check(Native.rwr_recommend_audience_set_long_batch(graph.handle, K, setPtr, setIdx, setW, dampingFactor, nIteration, candType.HasValue ? (int)candType.Value : -1, mask, excludeMembers ? 1 : 0, pool == null ? -1 : pool.Length, pool == null || pool.Length == 0 ? new int[1] : pool, denyPtr, denyIdx, topN, ids, scores, null, counts));
            var all = new List<KeyValuePair<long, double>>[K];
            for (int k = 0; k < K; k++) {
                all[k] = new List<KeyValuePair<long, double>>(counts[k]);
                for (int q = 0; q < counts[k]; q++) all[k].Add(new KeyValuePair<long, double>(ids[(long)k * topN + q], scores[(long)k * topN + q]));
            }
            return all;
        }

        // ... for one set
        public List<KeyValuePair<long, double>> AudienceSetLong(int[] members, float dampingFactor, int nIteration, double[] weights = null,
                                                                NodeType? candType = null, IEnumerable<EdgeType> exclEdgeTypes = null,
                                                                bool excludeMembers = false, int[] pool = null, int[] deny = null, int topN = 4096) {
            return AudienceSetLongBatch(new[] { members }, dampingFactor, nIteration, weights == null ? null : new[] { weights }, candType,
                                        exclEdgeTypes, excludeMembers, pool, deny == null ? null : new[] { deny }, topN)[0];
        }

        // ... and the 0-based position and the score of every test id in the sets' WHOLE audience lists
        // (rwr_recommend_audience_set_positions_batch): positions[k][j] / scores[k][j] answer testSets[k][j] (-1 / +0.0: not in
        // the list), listLen[k] is list k's length
        public long[][] AudienceSetPositionsBatch(int[][] sets, float dampingFactor, int nIteration, long[][] testSets, out double[][] scores,
                                                  out long[] listLen, double[][] weights = null, NodeType? candType = null,
                                                  IEnumerable<EdgeType> exclEdgeTypes = null, bool excludeMembers = false, int[] pool = null,
                                                  int[][] deny = null) {
            int K = sets.Length;
            if (testSets.Length != K) throw new System.ArgumentException("one test set per target set", "testSets");
            long[] setPtr, denyPtr; int[] setIdx, denyIdx; double[] setW; uint mask;
            PackAudienceSets(sets, weights, exclEdgeTypes, deny, out setPtr, out setIdx, out setW, out denyPtr, out denyIdx, out mask);
            var testPtr = new long[K + 1];
            var testIds = new List<long>();
            for (int k = 0; k < K; k++) { testIds.AddRange(testSets[k]); testPtr[k + 1] = testIds.Count; }
            int total = testIds.Count;
            testIds.Add(0);
            var pos = new long[total + 1]; var sc = new double[total + 1];
            listLen = new long[K];
            Native.Check(Native.rwr_recommend_audience_set_positions_batch(graph.handle, K, setPtr, setIdx, setW, dampingFactor, nIteration, candType.HasValue ? (int)candType.Value : -1, mask, excludeMembers ? 1 : 0, pool == null ? -1 : pool.Length, pool == null || pool.Length == 0 ? new int[1] : pool, denyPtr, denyIdx, testPtr, testIds.ToArray(), pos, sc, K == 0 ? new long[1] : listLen));
            var all = new long[K][];
            scores = new double[K][];
            for (int k = 0; k < K; k++) {
                int len = (int)(testPtr[k + 1] - testPtr[k]);
                all[k] = new long[len]; scores[k] = new double[len];
                System.Array.Copy(pos, testPtr[k], all[k], 0, len);
                System.Array.Copy(sc, testPtr[k], scores[k], 0, len);
            }
            return all;
        }

        // the arrays the audience set entries take: the sets and the deny lists as CSR (null where the caller gave none)
        static void PackAudienceSets(int[][] sets, double[][] weights, IEnumerable<EdgeType> exclEdgeTypes, int[][] deny, out long[] setPtr,
                                     out int[] setIdx, out double[] setW, out long[] denyPtr, out int[] denyIdx, out uint mask) {
            int K = sets.Length;
            if (weights != null && weights.Length != K) throw new System.ArgumentException("one weight list per set", "weights");
            if (deny != null && deny.Length != K) throw new System.ArgumentException("one deny list per set", "deny");
            mask = 0;
            if (exclEdgeTypes != null) foreach (var t in exclEdgeTypes) mask |= 1u << (int)t;
            setPtr = new long[K + 1];
            var idx = new List<int>(); var w = new List<double>(); var dn = new List<int>();
            denyPtr = deny == null ? null : new long[K + 1];
            for (int k = 0; k < K; k++) {
                if (weights != null && weights[k].Length != sets[k].Length) throw new System.ArgumentException("one weight per member", "weights");
                idx.AddRange(sets[k]);
                if (weights != null) w.AddRange(weights[k]);
                setPtr[k + 1] = idx.Count;
                if (deny != null) { dn.AddRange(deny[k]); denyPtr[k + 1] = dn.Count; }
            }
            idx.Add(0); w.Add(0.0); dn.Add(0);
            setIdx = idx.ToArray();
            setW = weights == null ? null : w.ToArray();
            denyIdx = deny == null ? null : dn.ToArray();
        }

        // addition: the top-N lists of K seeds among the nodes of ONE node type (rwr_recommend_typed_batch).  candType: the
        // candidates' type; exclEdgeTypes: the targets of the seed's raw links of these types are no candidates (null: none);
        // excludeSelf: neither is the seed.  "Who to follow" is (NodeType.USER, {FRIENDSHIP, FOLLOW}, true); (NodeType.ITEM,
        // {LIKE}, false) is RecommendationBatch
        public List<KeyValuePair<long, double>>[] RecommendationTypedBatch(int[] seeds, float dampingFactor, int nIteration, int topN,
                                                                           NodeType candType, IEnumerable<EdgeType> exclEdgeTypes = null,
                                                                           bool excludeSelf = false) {
            if (topN < 1) throw new System.ArgumentOutOfRangeException("topN", "RecommendationTypedBatch needs topN >= 1");
            int K = seeds.Length;
            uint mask = 0;
            if (exclEdgeTypes != null) foreach (var t in exclEdgeTypes) mask |= 1u << (int)t;
            var ids = new long[(long)K * topN]; var scores = new double[(long)K * topN]; var counts = new int[K];
            Native.Check(Native.rwr_recommend_typed_batch(graph.handle, seeds, K, dampingFactor, nIteration, topN, (int)candType, mask, excludeSelf ? 1 : 0, ids, scores, counts));
            var all = new List<KeyValuePair<long, double>>[K];
            for (int k = 0; k < K; k++) {
                all[k] = new List<KeyValuePair<long, double>>(counts[k]);
                for (int q = 0; q < counts[k]; q++) all[k].Add(new KeyValuePair<long, double>(ids[(long)k * topN + q], scores[(long)k * topN + q]));
            }
            return all;
        }

        // ... and for one seed
        public List<KeyValuePair<long, double>> RecommendationTyped(int idxTargetNode, float dampingFactor, int nIteration, int topN,
                                                                    NodeType candType, IEnumerable<EdgeType> exclEdgeTypes = null,
                                                                    bool excludeSelf = false) {
            return RecommendationTypedBatch(new[] { idxTargetNode }, dampingFactor, nIteration, topN, candType, exclEdgeTypes, excludeSelf)[0];
        }

        // addition: Hits and the running-precision sum (Experiment.cs:121-128) of K seeds' WHOLE lists among the nodes of one node
        // type against one test set each, evaluated on the device without writing a ranked list (rwr_recommend_typed_eval_batch).
        // candType, exclEdgeTypes and excludeSelf as in RecommendationTypedBatch; topN > 0 evaluates the first topN entries of
        // every list (any value), topN <= 0 the whole list
        public void RecommendationTypedEvalBatch(int[] seeds, float dampingFactor, int nIteration, HashSet<long>[] testSets,
                                                 NodeType candType, out long[] nHits, out double[] sumPrecision, out long[] listLen,
                                                 IEnumerable<EdgeType> exclEdgeTypes = null, bool excludeSelf = false, int topN = 0) {
            int K = seeds.Length;
            if (testSets.Length != K) throw new System.ArgumentException("testSets must hold one entry per seed");
            uint mask = 0;
            if (exclEdgeTypes != null) foreach (var t in exclEdgeTypes) mask |= 1u << (int)t;
            var testPtr = new long[K + 1];
            for (int k = 0; k < K; k++) testPtr[k + 1] = testPtr[k] + testSets[k].Count;
            var testIds = new long[testPtr[K]];
            for (int k = 0; k < K; k++) testSets[k].CopyTo(testIds, (int)testPtr[k]);
            nHits = new long[K]; sumPrecision = new double[K]; listLen = new long[K];
            Native.Check(Native.rwr_recommend_typed_eval_batch(graph.handle, seeds, K, dampingFactor, nIteration, topN, (int)candType, mask, excludeSelf ? 1 : 0, testPtr, testIds, nHits, sumPrecision, listLen));
        }

        // ... and for one seed
        public void RecommendationTypedEval(int idxTargetNode, float dampingFactor, int nIteration, HashSet<long> testSet,
                                            NodeType candType, out long nHits, out double sumPrecision, out long listLen,
                                            IEnumerable<EdgeType> exclEdgeTypes = null, bool excludeSelf = false, int topN = 0) {
            long[] h; double[] sp; long[] ln;
            RecommendationTypedEvalBatch(new[] { idxTargetNode }, dampingFactor, nIteration, new[] { testSet }, candType, out h, out sp, out ln,
                                         exclEdgeTypes, excludeSelf, topN);
            nHits = h[0]; sumPrecision = sp[0]; listLen = ln[0];
        }

        // K id arrays in the caller's order as CSR
        static void PackTests(long[][] testIds, int K, out long[] testPtr, out long[] flat) {
            if (testIds.Length != K) throw new System.ArgumentException("testIds must hold one entry per walk");
            testPtr = new long[K + 1];
            for (int k = 0; k < K; k++) testPtr[k + 1] = testPtr[k] + testIds[k].Length;
            flat = new long[testPtr[K]];
            for (int k = 0; k < K; k++) System.Array.Copy(testIds[k], 0, flat, testPtr[k], testIds[k].Length);
        }

        // ... and the flat result arrays of a positions entry cut back into K arrays aligned with them
        static void SplitTests(long[] testPtr, long[] pos, double[] score, out long[][] positions, out double[][] scores) {
            int K = testPtr.Length - 1;
            positions = new long[K][]; scores = new double[K][];
            for (int k = 0; k < K; k++) {
                long len = testPtr[k + 1] - testPtr[k];
                positions[k] = new long[len]; scores[k] = new double[len];
                System.Array.Copy(pos, testPtr[k], positions[k], 0, len);
                System.Array.Copy(score, testPtr[k], scores[k], 0, len);
            }
        }

        // addition: the 0-based position and the score of every test id in K seeds' WHOLE lists among the nodes of one node type,
        // found on the device by counting, no list written (rwr_recommend_typed_positions_batch).  positions[k][j] / scores[k][j]
        // answer testIds[k][j] -- the caller's order, duplicates kept; -1 / +0.0 where the list does not hold the id.  candType,
        // exclEdgeTypes and excludeSelf as in RecommendationTypedBatch.  MRR, NDCG@k, recall@k and AUC follow on the host
        public void RecommendationTypedPositionsBatch(int[] seeds, float dampingFactor, int nIteration, long[][] testIds,
                                                      NodeType candType, out long[][] positions, out double[][] scores,
                                                      out long[] listLen, IEnumerable<EdgeType> exclEdgeTypes = null,
                                                      bool excludeSelf = false) {
            int K = seeds.Length;
            uint mask = 0;
            if (exclEdgeTypes != null) foreach (var t in exclEdgeTypes) mask |= 1u << (int)t;
            long[] testPtr, flat;
            PackTests(testIds, K, out testPtr, out flat);
            var pos = new long[System.Math.Max(testPtr[K], 1)]; var score = new double[pos.Length]; listLen = new long[K];
            Native.Check(Native.rwr_recommend_typed_positions_batch(graph.handle, seeds, K, dampingFactor, nIteration, (int)candType, mask, excludeSelf ? 1 : 0, testPtr, flat, pos, score, listLen));
            SplitTests(testPtr, pos, score, out positions, out scores);
        }

        // ... and for one seed
        public void RecommendationTypedPositions(int idxTargetNode, float dampingFactor, int nIteration, long[] testIds,
                                                 NodeType candType, out long[] positions, out double[] scores, out long listLen,
                                                 IEnumerable<EdgeType> exclEdgeTypes = null, bool excludeSelf = false) {
            long[][] p; double[][] s; long[] ln;
            RecommendationTypedPositionsBatch(new[] { idxTargetNode }, dampingFactor, nIteration, new[] { testIds }, candType, out p, out s,
                                              out ln, exclEdgeTypes, excludeSelf);
            positions = p[0]; scores = s[0]; listLen = ln[0];
        }

        // K deny lists (node indices) as CSR; null: none
        static void PackDeny(int[][] deny, int K, out long[] denyPtr, out int[] denyIdx) {
            denyPtr = null; denyIdx = null;
            if (deny == null) return;
            if (deny.Length != K) throw new System.ArgumentException("deny must hold one entry per seed");
            denyPtr = new long[K + 1];
            for (int k = 0; k < K; k++) denyPtr[k + 1] = denyPtr[k] + deny[k].Length;
            denyIdx = new int[System.Math.Max(denyPtr[K], 1)];
            for (int k = 0; k < K; k++) System.Array.Copy(deny[k], 0, denyIdx, denyPtr[k], deny[k].Length);
        }

        // addition: the top-N lists of K seeds within a candidate pool the caller sets and with a deny list per seed
        // (rwr_recommend_filtered_batch).  candType: the candidates' type, null: nodes of any type; exclEdgeTypes and excludeSelf
        // as in RecommendationTypedBatch; pool: node INDICES in any order, duplicates allowed -- only these are ranked, for every
        // seed (null: no pool, an empty array: an empty pool, every list empty); deny[k]: node indices never shown to seed k
        // (null: none)
        public List<KeyValuePair<long, double>>[] RecommendationFilteredBatch(int[] seeds, float dampingFactor, int nIteration, int topN,
                                                                              NodeType? candType = null,
                                                                              IEnumerable<EdgeType> exclEdgeTypes = null,
                                                                              bool excludeSelf = false, int[] pool = null,
                                                                              int[][] deny = null) {
            if (topN < 1) throw new System.ArgumentOutOfRangeException("topN", "RecommendationFilteredBatch needs topN >= 1");
            int K = seeds.Length;
            uint mask = 0;
            if (exclEdgeTypes != null) foreach (var t in exclEdgeTypes) mask |= 1u << (int)t;
            long[] denyPtr; int[] denyIdx;
            PackDeny(deny, K, out denyPtr, out denyIdx);
            long poolCount = pool == null ? -1 : pool.Length;
            int[] poolIdx = (pool != null && pool.Length == 0) ? new int[1] : pool;
            var ids = new long[(long)K * topN]; var scores = new double[(long)K * topN]; var counts = new int[K];
            Native.Check(Native.rwr_recommend_filtered_batch(graph.handle, seeds, K, dampingFactor, nIteration, topN, candType.HasValue ? (int)candType.Value : -1, mask, excludeSelf ? 1 : 0, poolCount, poolIdx, denyPtr, denyIdx, ids, scores, counts));
            var all = new List<KeyValuePair<long, double>>[K];
            for (int k = 0; k < K; k++) {
                all[k] = new List<KeyValuePair<long, double>>(counts[k]);
                for (int q = 0; q < counts[k]; q++) all[k].Add(new KeyValuePair<long, double>(ids[(long)k * topN + q], scores[(long)k * topN + q]));
            }
            return all;
        }

        // ... and for one seed (deny: its one deny list)
        public List<KeyValuePair<long, double>> RecommendationFiltered(int idxTargetNode, float dampingFactor, int nIteration, int topN,
                                                                       NodeType? candType = null,
                                                                       IEnumerable<EdgeType> exclEdgeTypes = null,
                                                                       bool excludeSelf = false, int[] pool = null, int[] deny = null) {
            return RecommendationFilteredBatch(new[] { idxTargetNode }, dampingFactor, nIteration, topN, candType, exclEdgeTypes, excludeSelf,
                                               pool, deny == null ? null : new[] { deny })[0];
        }

        // addition: the 0-based position and the score of every test id in K seeds' WHOLE filtered lists
        // (rwr_recommend_filtered_positions_batch): RecommendationTypedPositionsBatch over the lists RecommendationFilteredBatch
        // defines.  A denied id, an id outside the pool and an id no node carries answer -1 / +0.0
        public void RecommendationFilteredPositionsBatch(int[] seeds, float dampingFactor, int nIteration, long[][] testIds,
                                                         out long[][] positions, out double[][] scores, out long[] listLen,
                                                         NodeType? candType = null, IEnumerable<EdgeType> exclEdgeTypes = null,
                                                         bool excludeSelf = false, int[] pool = null, int[][] deny = null) {
            int K = seeds.Length;
            uint mask = 0;
            if (exclEdgeTypes != null) foreach (var t in exclEdgeTypes) mask |= 1u << (int)t;
            long[] denyPtr; int[] denyIdx;
            PackDeny(deny, K, out denyPtr, out denyIdx);
            long poolCount = pool == null ? -1 : pool.Length;
            int[] poolIdx = (pool != null && pool.Length == 0) ? new int[1] : pool;
            long[] testPtr, flat;
            PackTests(testIds, K, out testPtr, out flat);
            var pos = new long[System.Math.Max(testPtr[K], 1)]; var score = new double[pos.Length]; listLen = new long[K];
            Native.Check(Native.rwr_recommend_filtered_positions_batch(graph.handle, seeds, K, dampingFactor, nIteration, candType.HasValue ? (int)candType.Value : -1, mask, excludeSelf ? 1 : 0, poolCount, poolIdx, denyPtr, denyIdx, testPtr, flat, pos, score, listLen));
            SplitTests(testPtr, pos, score, out positions, out scores);
        }

        // addition: RecommendationFilteredBatch with a diversity cap -- at most groupCap entries per group of nodes in every list
        // (rwr_recommend_capped_batch).  groupOf: one label per node of the graph (appended nodes included), any value >= 0 a
        // group, a negative value "never capped"; null: no cap, the filtered call.  groupCap in [1, 8].  Candidates the mask,
        // excludeSelf, the pool or a deny list remove do not use up a group's allowance
        public List<KeyValuePair<long, double>>[] RecommendationCappedBatch(int[] seeds, float dampingFactor, int nIteration, int topN,
                                                                            NodeType? candType = null,
                                                                            IEnumerable<EdgeType> exclEdgeTypes = null,
                                                                            bool excludeSelf = false, int[] pool = null,
                                                                            int[][] deny = null, int[] groupOf = null, int groupCap = 1) {
            if (topN < 1) throw new System.ArgumentOutOfRangeException("topN", "RecommendationCappedBatch needs topN >= 1");
            int K = seeds.Length;
            uint mask = 0;
            if (exclEdgeTypes != null) foreach (var t in exclEdgeTypes) mask |= 1u << (int)t;
            long[] denyPtr; int[] denyIdx;
            PackDeny(deny, K, out denyPtr, out denyIdx);
            long poolCount = pool == null ? -1 : pool.Length;
            int[] poolIdx = (pool != null && pool.Length == 0) ? new int[1] : pool;
            var ids = new long[(long)K * topN]; var scores = new double[(long)K * topN]; var counts = new int[K];
            Native.Check(Native.rwr_recommend_capped_batch(graph.handle, seeds, K, dampingFactor, nIteration, topN, candType.HasValue ? (int)candType.Value : -1, mask, excludeSelf ? 1 : 0, poolCount, poolIdx, denyPtr, denyIdx, groupOf, groupCap, ids, scores, counts));
            var all = new List<KeyValuePair<long, double>>[K];
            for (int k = 0; k < K; k++) {
                all[k] = new List<KeyValuePair<long, double>>(counts[k]);
                for (int q = 0; q < counts[k]; q++) all[k].Add(new KeyValuePair<long, double>(ids[(long)k * topN + q], scores[(long)k * topN + q]));
            }
            return all;
        }

        // ... and for one seed (deny: its one deny list)
        public List<KeyValuePair<long, double>> RecommendationCapped(int idxTargetNode, float dampingFactor, int nIteration, int topN,
                                                                     NodeType? candType = null,
                                                                     IEnumerable<EdgeType> exclEdgeTypes = null,
                                                                     bool excludeSelf = false, int[] pool = null, int[] deny = null,
                                                                     int[] groupOf = null, int groupCap = 1) {
            return RecommendationCappedBatch(new[] { idxTargetNode }, dampingFactor, nIteration, topN, candType, exclEdgeTypes, excludeSelf,
                                             pool, deny == null ? null : new[] { deny }, groupOf, groupCap)[0];
        }

        // addition: RecommendationCappedBatch for lists of up to 65 536 entries (rwr_recommend_long_batch): candidates for a
        // re-ranker.  The order is score descending, id descending, node index ascending; nodes[k * topN + j]: the node index of
        // entry j of seed k (-1 behind the list's end).  Up to 1 024 entries the call is the explained call without reasons
        public List<KeyValuePair<long, double>>[] RecommendationLongBatch(int[] seeds, float dampingFactor, int nIteration, int topN,
                                                                          out int[] nodes, NodeType? candType = null,
                                                                          IEnumerable<EdgeType> exclEdgeTypes = null,
                                                                          bool excludeSelf = false, int[] pool = null,
                                                                          int[][] deny = null, int[] groupOf = null, int groupCap = 1) {
            if (topN < 1 || topN > 65536) throw new System.ArgumentOutOfRangeException("topN", "RecommendationLongBatch needs topN in [1, 65536]");
            int K = seeds.Length;
            uint mask = 0;
            if (exclEdgeTypes != null) foreach (var t in exclEdgeTypes) mask |= 1u << (int)t;
            long[] denyPtr; int[] denyIdx;
            PackDeny(deny, K, out denyPtr, out denyIdx);
            long poolCount = pool == null ? -1 : pool.Length;
            int[] poolIdx = (pool != null && pool.Length == 0) ? new int[1] : pool;
            var ids = new long[(long)K * topN]; var scores = new double[(long)K * topN]; var counts = new int[K];
            nodes = new int[(long)K * topN];
            Native.Check(Native.rwr_recommend_long_batch(graph.handle, seeds, K, dampingFactor, nIteration, topN, candType.HasValue ? (int)candType.Value : -1, mask, excludeSelf ? 1 : 0, poolCount, poolIdx, denyPtr, denyIdx, groupOf, groupCap, ids, scores, counts, nodes));
            var all = new List<KeyValuePair<long, double>>[K];
            for (int k = 0; k < K; k++) {
                all[k] = new List<KeyValuePair<long, double>>(counts[k]);
                for (int q = 0; q < counts[k]; q++) all[k].Add(new KeyValuePair<long, double>(ids[(long)k * topN + q], scores[(long)k * topN + q]));
            }
            return all;
        }

        // ... and for one seed (deny: its one deny list)
        public List<KeyValuePair<long, double>> RecommendationLong(int idxTargetNode, float dampingFactor, int nIteration, int topN,
                                                                   NodeType? candType = null, IEnumerable<EdgeType> exclEdgeTypes = null,
                                                                   bool excludeSelf = false, int[] pool = null, int[] deny = null,
                                                                   int[] groupOf = null, int groupCap = 1) {
            int[] nodes;
            return RecommendationLongBatch(new[] { idxTargetNode }, dampingFactor, nIteration, topN, out nodes, candType, exclEdgeTypes,
                                           excludeSelf, pool, deny == null ? null : new[] { deny }, groupOf, groupCap)[0];
        }

        // addition: RecommendationCappedBatch with the reasons of every list entry (rwr_recommend_explained_batch).  nodes[k * topN + j]:
        // the node index of entry j of seed k (-1 behind the list's end); whySrc / whyTerm[(k * topN + j) * nWhy + i]: the source node
        // and the value of the entry's i-th largest in-link addend fl(fl((1 - d) * previousRank[u]) * weight(u -> v)) (-1 / +0.0
        // where fewer are positive); whyTotal[k * topN + j]: the number of positive addends.  nWhy in [0, 8]
        public List<KeyValuePair<long, double>>[] RecommendationExplainedBatch(int[] seeds, float dampingFactor, int nIteration, int topN,
                                                                               int nWhy, out int[] nodes, out int[] whySrc,
                                                                               out double[] whyTerm, out long[] whyTotal,
                                                                               NodeType? candType = null,
                                                                               IEnumerable<EdgeType> exclEdgeTypes = null,
                                                                               bool excludeSelf = false, int[] pool = null,
                                                                               int[][] deny = null, int[] groupOf = null, int groupCap = 1) {
            if (topN < 1) throw new System.ArgumentOutOfRangeException("topN", "RecommendationExplainedBatch needs topN >= 1");
            if (nWhy < 0 || nWhy > 8) throw new System.ArgumentOutOfRangeException("nWhy", "RecommendationExplainedBatch needs nWhy in [0, 8]");
            int K = seeds.Length;
            uint mask = 0;
            if (exclEdgeTypes != null) foreach (var t in exclEdgeTypes) mask |= 1u << (int)t;
            long[] denyPtr; int[] denyIdx;
            PackDeny(deny, K, out denyPtr, out denyIdx);
            long poolCount = pool == null ? -1 : pool.Length;
            int[] poolIdx = (pool != null && pool.Length == 0) ? new int[1] : pool;
            var ids = new long[(long)K * topN]; var scores = new double[(long)K * topN]; var counts = new int[K];
            nodes = new int[(long)K * topN]; whyTotal = new long[(long)K * topN];
            whySrc = new int[(long)K * topN * nWhy + 1]; whyTerm = new double[(long)K * topN * nWhy + 1];
            Native.Check(Native.rwr_recommend_explained_batch(graph.handle, seeds, K, dampingFactor, nIteration, topN, candType.HasValue ? (int)candType.Value : -1, mask, excludeSelf ? 1 : 0, poolCount, poolIdx, denyPtr, denyIdx, groupOf, groupCap, nWhy, ids, scores, counts, nodes, whySrc, whyTerm, whyTotal));
            System.Array.Resize(ref whySrc, K * topN * nWhy); System.Array.Resize(ref whyTerm, K * topN * nWhy);
            var all = new List<KeyValuePair<long, double>>[K];
            for (int k = 0; k < K; k++) {
                all[k] = new List<KeyValuePair<long, double>>(counts[k]);
                for (int q = 0; q < counts[k]; q++) all[k].Add(new KeyValuePair<long, double>(ids[(long)k * topN + q], scores[(long)k * topN + q]));
            }
            return all;
        }

        // ... and for one seed (deny: its one deny list)
        public List<KeyValuePair<long, double>> RecommendationExplained(int idxTargetNode, float dampingFactor, int nIteration, int topN,
                                                                        int nWhy, out int[] nodes, out int[] whySrc, out double[] whyTerm,
                                                                        out long[] whyTotal, NodeType? candType = null,
                                                                        IEnumerable<EdgeType> exclEdgeTypes = null,
                                                                        bool excludeSelf = false, int[] pool = null, int[] deny = null,
                                                                        int[] groupOf = null, int groupCap = 1) {
            return RecommendationExplainedBatch(new[] { idxTargetNode }, dampingFactor, nIteration, topN, nWhy, out nodes, out whySrc,
                                                out whyTerm, out whyTotal, candType, exclEdgeTypes, excludeSelf, pool,
                                                deny == null ? null : new[] { deny }, groupOf, groupCap)[0];
        }

        // addition: the 0-based position and the score of every test id in K seeds' WHOLE capped lists
        // (rwr_recommend_capped_positions_batch): RecommendationFilteredPositionsBatch over the lists RecommendationCappedBatch
        // defines.  An id the cap drops answers -1 / +0.0, like a denied one; listLen[k] is the capped list's length
        public void RecommendationCappedPositionsBatch(int[] seeds, float dampingFactor, int nIteration, long[][] testIds,
                                                       out long[][] positions, out double[][] scores, out long[] listLen,
                                                       NodeType? candType = null, IEnumerable<EdgeType> exclEdgeTypes = null,
                                                       bool excludeSelf = false, int[] pool = null, int[][] deny = null,
                                                       int[] groupOf = null, int groupCap = 1) {
            int K = seeds.Length;
            uint mask = 0;
            if (exclEdgeTypes != null) foreach (var t in exclEdgeTypes) mask |= 1u << (int)t;
            long[] denyPtr; int[] denyIdx;
            PackDeny(deny, K, out denyPtr, out denyIdx);
            long poolCount = pool == null ? -1 : pool.Length;
            int[] poolIdx = (pool != null && pool.Length == 0) ? new int[1] : pool;
            long[] testPtr, flat;
            PackTests(testIds, K, out testPtr, out flat);
            var pos = new long[System.Math.Max(testPtr[K], 1)]; var score = new double[pos.Length]; listLen = new long[K];
            Native.Check(Native.rwr_recommend_capped_positions_batch(graph.handle, seeds, K, dampingFactor, nIteration, candType.HasValue ? (int)candType.Value : -1, mask, excludeSelf ? 1 : 0, poolCount, poolIdx, denyPtr, denyIdx, groupOf, groupCap, testPtr, flat, pos, score, listLen));
            SplitTests(testPtr, pos, score, out positions, out scores);
        }

        // addition: the same for K walks with caller-set restart vectors, in the whole lists RecommendationRestartTypedBatch defines
        // (rwr_recommend_restart_typed_positions_batch).  nodes, weights, start, candType, exclEdgeTypes, excludeMembers and
        // exclude as there
        public void RecommendationRestartTypedPositionsBatch(int[][] nodes, double[][] weights, int[] start, double dampingFactor,
                                                             int nIteration, long[][] testIds, NodeType candType,
                                                             out long[][] positions, out double[][] scores, out long[] listLen,
                                                             IEnumerable<EdgeType> exclEdgeTypes = null, bool excludeMembers = false,
                                                             int[][] exclude = null) {
            int K = nodes.Length;
            if (weights.Length != K || (start != null && start.Length != K) || (exclude != null && exclude.Length != K))
                throw new System.ArgumentException("nodes, weights, start and exclude must hold one entry per vector");
            uint mask = 0;
            if (exclEdgeTypes != null) foreach (var t in exclEdgeTypes) mask |= 1u << (int)t;
            var ptr = new long[K + 1];
            for (int k = 0; k < K; k++) {
                if (nodes[k].Length != weights[k].Length)
                    throw new System.ArgumentException("a restart vector's nodes and weights differ in length");
                ptr[k + 1] = ptr[k] + nodes[k].Length;
            }
            var idx = new int[ptr[K]];
            var val = new double[ptr[K]];
            for (int k = 0; k < K; k++) {
                System.Array.Copy(nodes[k], 0, idx, ptr[k], nodes[k].Length);
                System.Array.Copy(weights[k], 0, val, ptr[k], weights[k].Length);
            }
            long[] exclPtr = null;
            int[] exclIdx = null;
            if (exclude != null) {
                exclPtr = new long[K + 1];
                for (int k = 0; k < K; k++) exclPtr[k + 1] = exclPtr[k] + exclude[k].Length;
                exclIdx = new int[exclPtr[K]];
                for (int k = 0; k < K; k++) System.Array.Copy(exclude[k], 0, exclIdx, exclPtr[k], exclude[k].Length);
            }
            long[] testPtr, flat;
            PackTests(testIds, K, out testPtr, out flat);
            var pos = new long[System.Math.Max(testPtr[K], 1)]; var score = new double[pos.Length]; listLen = new long[K];
            Native.Check(Native.rwr_recommend_restart_typed_positions_batch(graph.handle, K, ptr, idx, val, start, exclPtr, exclIdx, dampingFactor, nIteration, (int)candType, mask, excludeMembers ? 1 : 0, testPtr, flat, pos, score, listLen));
            SplitTests(testPtr, pos, score, out positions, out scores);
        }

        // addition: the top-N lists of K walks with caller-set restart vectors among the nodes of ONE node type
        // (rwr_recommend_restart_typed_batch).  nodes, weights, start and exclude as in RecommendationRestartBatch; candType and
        // exclEdgeTypes as in RecommendationTypedBatch, applied to every member of exclusion set k; excludeMembers: the members
        // themselves are no candidates.  "Whom should this group follow" is (NodeType.USER, {FRIENDSHIP, FOLLOW}, true)
        public List<KeyValuePair<long, double>>[] RecommendationRestartTypedBatch(int[][] nodes, double[][] weights, int[] start,
                                                                                  double dampingFactor, int nIteration, int topN,
                                                                                  NodeType candType,
                                                                                  IEnumerable<EdgeType> exclEdgeTypes = null,
                                                                                  bool excludeMembers = false, int[][] exclude = null) {
            if (topN < 1) throw new System.ArgumentOutOfRangeException("topN", "RecommendationRestartTypedBatch needs topN >= 1");
            int K = nodes.Length;
            if (weights.Length != K || (start != null && start.Length != K) || (exclude != null && exclude.Length != K))
                throw new System.ArgumentException("nodes, weights, start and exclude must hold one entry per vector");
            uint mask = 0;
            if (exclEdgeTypes != null) foreach (var t in exclEdgeTypes) mask |= 1u << (int)t;
            var ptr = new long[K + 1];
            for (int k = 0; k < K; k++) {
                if (nodes[k].Length != weights[k].Length)
                    throw new System.ArgumentException("a restart vector's nodes and weights differ in length");
                ptr[k + 1] = ptr[k] + nodes[k].Length;
            }
            var idx = new int[ptr[K]];
            var val = new double[ptr[K]];
            for (int k = 0; k < K; k++) {
                System.Array.Copy(nodes[k], 0, idx, ptr[k], nodes[k].Length);
                System.Array.Copy(weights[k], 0, val, ptr[k], weights[k].Length);
            }
            long[] exclPtr = null;
            int[] exclIdx = null;
            if (exclude != null) {
                exclPtr = new long[K + 1];
                for (int k = 0; k < K; k++) exclPtr[k + 1] = exclPtr[k] + exclude[k].Length;
                exclIdx = new int[exclPtr[K]];
                for (int k = 0; k < K; k++) System.Array.Copy(exclude[k], 0, exclIdx, exclPtr[k], exclude[k].Length);
            }
            var ids = new long[(long)K * topN]; var scores = new double[(long)K * topN]; var counts = new int[K];
            Native.Check(Native.rwr_recommend_restart_typed_batch(graph.handle, K, ptr, idx, val, start, exclPtr, exclIdx, dampingFactor, nIteration, topN, (int)candType, mask, excludeMembers ? 1 : 0, ids, scores, counts));
            var all = new List<KeyValuePair<long, double>>[K];
            for (int k = 0; k < K; k++) {
                all[k] = new List<KeyValuePair<long, double>>(counts[k]);
                for (int q = 0; q < counts[k]; q++) all[k].Add(new KeyValuePair<long, double>(ids[(long)k * topN + q], scores[(long)k * topN + q]));
            }
            return all;
        }

        // addition: the top-N lists of K walks with caller-set restart vectors (Model.restart), ranked on the device
        // (rwr_recommend_restart_batch).  Vector k has restart[nodes[k][j]] = weights[k][j] >= 0 and zero elsewhere; start as in
        // Model.RunRestartBatch.  exclude[k]: the nodes whose LIKEd items are not candidates of vector k (Recommender.cs:20-24
        // for each of them); exclude == null: the nodes of vector k's own support.  List k is what ranking the rank of that
        // Model after run(nIteration) gives
        public List<KeyValuePair<long, double>>[] RecommendationRestartBatch(int[][] nodes, double[][] weights, int[] start,
                                                                             double dampingFactor, int nIteration, int topN,
                                                                             int[][] exclude = null) {
            if (topN < 1) throw new System.ArgumentOutOfRangeException("topN", "RecommendationRestartBatch needs topN >= 1");
            int K = nodes.Length;
            if (weights.Length != K || (start != null && start.Length != K) || (exclude != null && exclude.Length != K))
                throw new System.ArgumentException("nodes, weights, start and exclude must hold one entry per vector");
            var ptr = new long[K + 1];
            for (int k = 0; k < K; k++) {
                if (nodes[k].Length != weights[k].Length)
                    throw new System.ArgumentException("a restart vector's nodes and weights differ in length");
                ptr[k + 1] = ptr[k] + nodes[k].Length;
            }
            var idx = new int[ptr[K]];
            var val = new double[ptr[K]];
            for (int k = 0; k < K; k++) {
                System.Array.Copy(nodes[k], 0, idx, ptr[k], nodes[k].Length);
                System.Array.Copy(weights[k], 0, val, ptr[k], weights[k].Length);
            }
            long[] exclPtr = null;
            int[] exclIdx = null;
            if (exclude != null) {
                exclPtr = new long[K + 1];
                for (int k = 0; k < K; k++) exclPtr[k + 1] = exclPtr[k] + exclude[k].Length;
                exclIdx = new int[exclPtr[K]];
                for (int k = 0; k < K; k++) System.Array.Copy(exclude[k], 0, exclIdx, exclPtr[k], exclude[k].Length);
            }
            var ids = new long[(long)K * topN]; var scores = new double[(long)K * topN]; var counts = new int[K];
            Native.Check(Native.rwr_recommend_restart_batch(graph.handle, K, ptr, idx, val, start, exclPtr, exclIdx, dampingFactor,
                                                            nIteration, topN, ids, scores, counts));
            var all = new List<KeyValuePair<long, double>>[K];
            for (int k = 0; k < K; k++) {
                all[k] = new List<KeyValuePair<long, double>>(counts[k]);
                for (int q = 0; q < counts[k]; q++) all[k].Add(new KeyValuePair<long, double>(ids[(long)k * topN + q], scores[(long)k * topN + q]));
            }
            return all;
        }

        // addition: Hits and the running-precision sum (Experiment.cs:121-128) of the same K walks against one test set each,
        // evaluated on the device without writing a ranked list (rwr_recommend_restart_eval_batch).  nodes, weights, start and
        // exclude as in RecommendationRestartBatch; topN > 0 evaluates the first topN entries of every list, topN <= 0 the whole
        // list.  nHits[k] / sumPrecision[k] / listLen[k] are what the harness computes over list k
        public void RecommendationRestartEvalBatch(int[][] nodes, double[][] weights, int[] start, double dampingFactor,
                                                   int nIteration, HashSet<long>[] testSets, out long[] nHits,
                                                   out double[] sumPrecision, out long[] listLen, int topN = 0,
                                                   int[][] exclude = null) {
            int K = nodes.Length;
            if (weights.Length != K || testSets.Length != K || (start != null && start.Length != K) ||
                (exclude != null && exclude.Length != K))
                throw new System.ArgumentException("nodes, weights, start, testSets and exclude must hold one entry per vector");
            var ptr = new long[K + 1];
            for (int k = 0; k < K; k++) {
                if (nodes[k].Length != weights[k].Length)
                    throw new System.ArgumentException("a restart vector's nodes and weights differ in length");
                ptr[k + 1] = ptr[k] + nodes[k].Length;
            }
            var idx = new int[ptr[K]];
            var val = new double[ptr[K]];
            for (int k = 0; k < K; k++) {
                System.Array.Copy(nodes[k], 0, idx, ptr[k], nodes[k].Length);
                System.Array.Copy(weights[k], 0, val, ptr[k], weights[k].Length);
            }
            long[] exclPtr = null;
            int[] exclIdx = null;
            if (exclude != null) {
                exclPtr = new long[K + 1];
                for (int k = 0; k < K; k++) exclPtr[k + 1] = exclPtr[k] + exclude[k].Length;
                exclIdx = new int[exclPtr[K]];
                for (int k = 0; k < K; k++) System.Array.Copy(exclude[k], 0, exclIdx, exclPtr[k], exclude[k].Length);
            }
            var testPtr = new long[K + 1];
            for (int k = 0; k < K; k++) testPtr[k + 1] = testPtr[k] + testSets[k].Count;
            var testIds = new long[testPtr[K]];
            for (int k = 0; k < K; k++) testSets[k].CopyTo(testIds, (int)testPtr[k]);
            nHits = new long[K]; sumPrecision = new double[K]; listLen = new long[K];
            Native.Check(Native.rwr_recommend_restart_eval_batch(graph.handle, K, ptr, idx, val, start, exclPtr, exclIdx, dampingFactor,
                                                                 nIteration, topN, testPtr, testIds, nHits, sumPrecision, listLen));
        }
    }
}
