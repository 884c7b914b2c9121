// Drop-in replacement of Recommenders/RWRBased/Graph.cs of the reference: same public types, fields and
// methods (Node, ForwardLink, Graph{nodes, edges, graph, buildGraph(), size()}), so TweetRecommender/*.cs
// compile unchanged.  buildGraph() flattens the caller's dictionaries in list order and hands the RAW links
// to librwr, which filters / normalises / transposes on the GPU.
using System.Collections.Generic;

namespace Recommenders.RWRBased {
    public class Graph {
        public Dictionary<int, Node> nodes;
        public Dictionary<int, List<ForwardLink>> edges;
        // PUBLIC FIELD as in the reference (Graph.cs:43).  The harness never reads it (Experiment.cs:104-109 only calls
        // buildGraph and Recommendation), and filling it costs two blocking device-to-host copies plus one ForwardLink[] per
        // node on EVERY per-fold rebuild -- more than the device build itself for an ego network.  So it is opt-in: a host
        // that does read the field sets GraphFieldLimit to the largest link count it wants filled eagerly by buildGraph()
        // (a field cannot be materialised lazily), or calls LoadNormalizedGraph() when it needs it.  Default 0 = never.
        public Dictionary<int, ForwardLink[]> graph;
        public static long GraphFieldLimit = 0;
        internal GraphHandle handle;
        long[] rowptr; int[] dst; byte[] etype;
        long[] sentId; byte[] sentType; double[] sentW;   // what the device currently holds (for incremental rebuilds)
        bool sentInOrder;   // the node dictionary enumerated its keys as 0, 1, ..., n-1 when that record was taken
        // buildGraph() calls (all instances) that went through rwr_graph_append_nodes: nodes added at the end, lists that only grew
        public static long NodeAppendRebuilds = 0;

        public Graph(Dictionary<int, Node> nodes, Dictionary<int, List<ForwardLink>> edges) {
            this.nodes = nodes;
            this.edges = edges;
        }

        public void buildGraph() {
            int n = nodes.Count;
            var id = new long[n]; var type = new byte[n];
            long[] prevRowptr = rowptr; int[] prevDst = dst; byte[] prevEtype = etype;
            rowptr = new long[n + 1];
            for (int i = 0; i < n; i++) {
                id[i] = nodes[i].id; type[i] = (byte)nodes[i].type;
                rowptr[i + 1] = rowptr[i] + (edges.ContainsKey(i) ? edges[i].Count : 0);
            }
            long m = rowptr[n];
            dst = new int[m]; etype = new byte[m]; var w = new double[m];
            long e = 0;
            for (int i = 0; i < n; i++) {
                if (!edges.ContainsKey(i)) continue;
                foreach (ForwardLink l in edges[i]) { dst[e] = l.targetNode; etype[e] = (byte)l.type; w[e] = l.weight; e++; }
            }
            graph = null;
            // buildGraph() called again on the same object after the host mutated link types or weights in place
            // (Experiment.cs:84-101 relabels FRIENDSHIP -> UNDEFINED): same nodes, same list lengths, same targets
            // => send only the links that differ (rwr_graph_update_links); the device state is identical either way.
            if (handle != null && !handle.IsInvalid && sentW != null && SameTopology(id, type, prevRowptr, prevDst)) {
                var idx = new List<long>(); var nt = new List<byte>(); var nw = new List<double>();
                for (long p = 0; p < m; p++)
                    if (etype[p] != prevEtype[p] || System.BitConverter.DoubleToInt64Bits(w[p]) != System.BitConverter.DoubleToInt64Bits(sentW[p])) {
                        idx.Add(p); nt.Add(etype[p]); nw.Add(w[p]);
                    }
                Native.Check(Native.rwr_graph_update_links(handle, idx.Count, idx.ToArray(), nt.ToArray(), nw.ToArray()));
            } else if (handle != null && !handle.IsInvalid && sentW != null && GrownLists(id, type, prevRowptr, prevDst, prevEtype, w)) {
                // same nodes, every old list a bitwise prefix of the new one => send only the new links (rwr_graph_append_links)
                var asrc = new List<int>(); var adst = new List<int>(); var at = new List<byte>(); var aw = new List<double>();
                for (int i = 0; i < n; i++)
                    for (long p = rowptr[i] + (prevRowptr[i + 1] - prevRowptr[i]); p < rowptr[i + 1]; p++) {
                        asrc.Add(i); adst.Add(dst[p]); at.Add(etype[p]); aw.Add(w[p]);
                    }
                Native.Check(Native.rwr_graph_append_links(handle, asrc.Count, asrc.ToArray(), adst.ToArray(), at.ToArray(), aw.ToArray(), null));
            } else if (handle != null && !handle.IsInvalid && sentW != null && sentInOrder && KeysInOrder() &&
                       GrownNodes(id, type, prevRowptr, prevDst, prevEtype, w)) {
                // the node dictionary only gained keys at its end (old nodes unchanged and in the same order, the new keys
                // continuing the index sequence), every old list a bitwise prefix of the new one => send only the new nodes
                // and the new links (rwr_graph_append_nodes); the lists of the new nodes start empty
                int nOld = sentId.Length;
                var nid = new long[n - nOld]; var nty = new byte[n - nOld];
                for (int j = 0; j < n - nOld; j++) { nid[j] = id[nOld + j]; nty[j] = type[nOld + j]; }
                var asrc = new List<int>(); var adst = new List<int>(); var at = new List<byte>(); var aw = new List<double>();
                for (int i = 0; i < n; i++) {
                    long kept = i < nOld ? prevRowptr[i + 1] - prevRowptr[i] : 0;
                    for (long p = rowptr[i] + kept; p < rowptr[i + 1]; p++) { asrc.Add(i); adst.Add(dst[p]); at.Add(etype[p]); aw.Add(w[p]); }
                }
                Native.Check(Native.rwr_graph_append_nodes(handle, n - nOld, nid, nty, asrc.Count, asrc.ToArray(), adst.ToArray(),
                                                           at.ToArray(), aw.ToArray(), null));
                NodeAppendRebuilds++;
            } else {
                var opts = new RwrOpts { struct_size = 40, device = -1, mode = -1 };
                Native.Check(Native.rwr_graph_create(n, id, type, rowptr, dst, etype, w, ref opts, out handle));
            }
            sentId = id; sentType = type; sentW = w;
            sentInOrder = KeysInOrder();
            if (GraphFieldLimit > 0 && m <= GraphFieldLimit) LoadNormalizedGraph();
        }

        // rwr_graph_append_links on a built graph: link q goes to the end of edges[src[q]] ON THE DEVICE (what
        // edges[src].Add(new ForwardLink(...)) does to the list, Graph.cs:40); returns the positions of the new links in the new
        // flattened raw list (for rwr_graph_update_links).  The dictionaries are not touched: add the same links to `edges`, and
        // the next buildGraph() finds nothing more to send.
        public long[] AppendLinks(int[] src, ForwardLink[] links) {
            if (src.Length != links.Length) throw new System.ArgumentException("one source per link");
            int n = nodes.Count, count = src.Length;
            var ad = new int[count]; var at = new byte[count]; var aw = new double[count]; var pos = new long[count];
            for (int q = 0; q < count; q++) { ad[q] = links[q].targetNode; at[q] = (byte)links[q].type; aw[q] = links[q].weight; }
            Native.Check(Native.rwr_graph_append_links(handle, count, src, ad, at, aw, pos));
            // the flat copies behind LoadNormalizedGraph() and the next buildGraph()'s diff follow
            var add = new long[n + 1];
            foreach (int s in src) add[s + 1]++;
            for (int i = 0; i < n; i++) add[i + 1] += add[i];
            var rp = new long[n + 1];
            for (int i = 0; i <= n; i++) rp[i] = rowptr[i] + add[i];
            var nd = new int[rp[n]]; var nt = new byte[rp[n]]; var nw = new double[rp[n]];
            for (int i = 0; i < n; i++)
                for (long p = rowptr[i]; p < rowptr[i + 1]; p++) { nd[p + add[i]] = dst[p]; nt[p + add[i]] = etype[p]; nw[p + add[i]] = sentW[p]; }
            for (int q = 0; q < count; q++) { nd[pos[q]] = ad[q]; nt[pos[q]] = at[q]; nw[pos[q]] = aw[q]; }
            rowptr = rp; dst = nd; etype = nt; sentW = nw;
            graph = null;
            return pos;
        }

        // rwr_graph_remove_links on a built graph: the raw links at the given flattened positions (distinct, any order) leave
        // their lists ON THE DEVICE (what edges[src].RemoveAt(k) does to the list); the surviving link at old position e is
        // afterwards at e - (removed positions < e).  The dictionaries are not touched: remove the same links from `edges`, and
        // the next buildGraph() finds nothing more to send.  (Deleting from `edges` WITHOUT this call makes buildGraph() send
        // the graph whole in this binding: only the Python mirror finds removed links by a list diff.)
        public void RemoveLinks(long[] linkIndex) {
            int n = nodes.Count;
            Native.Check(Native.rwr_graph_remove_links(handle, linkIndex.Length, linkIndex));
            // the flat copies behind LoadNormalizedGraph() and the next buildGraph()'s diff follow
            long m = rowptr[n];
            var gone = new bool[m];
            foreach (long p in linkIndex) gone[p] = true;
            var rp = new long[n + 1];
            var nd = new int[m - linkIndex.Length]; var nt = new byte[m - linkIndex.Length]; var nw = new double[m - linkIndex.Length];
            long f = 0;
            for (int i = 0; i < n; i++) {
                for (long p = rowptr[i]; p < rowptr[i + 1]; p++)
                    if (!gone[p]) { nd[f] = dst[p]; nt[f] = etype[p]; nw[f] = sentW[p]; f++; }
                rp[i + 1] = f;
            }
            rowptr = rp; dst = nd; etype = nt; sentW = nw;
            graph = null;
        }

        // rwr_graph_append_nodes on a built graph: node j of `added` gets index nodes.Count + j and an empty list ON THE DEVICE
        // (nodes.Add(n + j, ...); edges.Add(n + j, new List<ForwardLink>()), Graph.cs:39-40), then the links are appended as
        // AppendLinks appends them, src and targets ranging over the grown node set; one device-side rebuild for both.  Returns
        // the positions of the new links; the first new node has index nodes.Count.  The dictionaries are not touched: add the
        // same nodes and links to `nodes` / `edges` BEFORE any other call on this object (it reads nodes.Count), and the next
        // buildGraph() finds nothing more to send.
        public long[] AppendNodes(Node[] added, int[] src, ForwardLink[] links) {
            if (src.Length != links.Length) throw new System.ArgumentException("one source per link");
            int nOld = sentId.Length, k = added.Length, n = nOld + k, count = src.Length;
            var nid = new long[k]; var nty = new byte[k];
            for (int j = 0; j < k; j++) { nid[j] = added[j].id; nty[j] = (byte)added[j].type; }
            var ad = new int[count]; var at = new byte[count]; var aw = new double[count]; var pos = new long[count];
            for (int q = 0; q < count; q++) { ad[q] = links[q].targetNode; at[q] = (byte)links[q].type; aw[q] = links[q].weight; }
            Native.Check(Native.rwr_graph_append_nodes(handle, k, nid, nty, count, src, ad, at, aw, pos));
            // the flat copies behind LoadNormalizedGraph() and the next buildGraph()'s diff follow
            var id2 = new long[n]; var ty2 = new byte[n];
            for (int i = 0; i < nOld; i++) { id2[i] = sentId[i]; ty2[i] = sentType[i]; }
            for (int j = 0; j < k; j++) { id2[nOld + j] = nid[j]; ty2[nOld + j] = nty[j]; }
            var add = new long[n + 1];
            foreach (int s in src) add[s + 1]++;
            for (int i = 0; i < n; i++) add[i + 1] += add[i];
            var rp = new long[n + 1];
            for (int i = 0; i <= n; i++) rp[i] = rowptr[i < nOld ? i : nOld] + add[i];
            var nd = new int[rp[n]]; var nt = new byte[rp[n]]; var nw = new double[rp[n]];
            for (int i = 0; i < nOld; i++)
                for (long p = rowptr[i]; p < rowptr[i + 1]; p++) { nd[p + add[i]] = dst[p]; nt[p + add[i]] = etype[p]; nw[p + add[i]] = sentW[p]; }
            for (int q = 0; q < count; q++) { nd[pos[q]] = ad[q]; nt[pos[q]] = at[q]; nw[pos[q]] = aw[q]; }
            rowptr = rp; dst = nd; etype = nt; sentW = nw; sentId = id2; sentType = ty2;
            graph = null;
            return pos;
        }

        // rwr_graph_remove_nodes on a built graph: the nodes at the given indices (distinct, any order) leave the graph ON THE
        // DEVICE with every raw link from or to them (nodes.Remove(i); edges.Remove(i), and the links to i out of the other
        // lists); the others close up and keep their order.  newNodeIndex[i] is the new index of old node i and
        // newLinkIndex[e] the new position of the link at old flattened position e, -1 for what left.  The dictionaries are
        // not touched: take the same nodes and links out of `nodes` / `edges` and re-key both by newNodeIndex BEFORE any other
        // call on this object (it reads nodes.Count), and the next buildGraph() finds nothing more to send.  (Removing nodes
        // from the dictionaries WITHOUT this call makes buildGraph() send the graph whole in this binding: only the Python
        // mirror finds lost nodes by a diff.)
        public void RemoveNodes(int[] nodeIndex, out int[] newNodeIndex, out long[] newLinkIndex) {
            int nOld = sentId.Length;
            long m = rowptr[nOld];
            newNodeIndex = new int[nOld]; newLinkIndex = new long[m];
            long removed;
            Native.Check(Native.rwr_graph_remove_nodes(handle, nodeIndex.Length, nodeIndex, newNodeIndex, newLinkIndex, out removed));
            // the flat copies behind LoadNormalizedGraph() and the next buildGraph()'s diff follow
            int n = nOld - nodeIndex.Length;
            var id2 = new long[n]; var ty2 = new byte[n]; var rp = new long[n + 1];
            var nd = new int[m - removed]; var nt = new byte[m - removed]; var nw = new double[m - removed];
            for (int i = 0; i < nOld; i++) {
                int to = newNodeIndex[i];
                if (to < 0) continue;
                id2[to] = sentId[i]; ty2[to] = sentType[i];
                long f = rp[to];
                for (long p = rowptr[i]; p < rowptr[i + 1]; p++)
                    if (newLinkIndex[p] >= 0) { nd[f] = newNodeIndex[dst[p]]; nt[f] = etype[p]; nw[f] = sentW[p]; f++; }
                rp[to + 1] = f;
            }
            rowptr = rp; dst = nd; etype = nt; sentW = nw; sentId = id2; sentType = ty2;
            graph = null;
        }

        // the flat arrays buildGraph() hands to librwr, without building: Recommender.EvaluateGraphs sends many graphs at once
        internal void Flatten(out long[] id, out byte[] type, out long[] rp, out int[] d, out byte[] et, out double[] w) {
            int n = nodes.Count;
            id = new long[n]; type = new byte[n]; rp = new long[n + 1];
            for (int i = 0; i < n; i++) {
                id[i] = nodes[i].id; type[i] = (byte)nodes[i].type;
                rp[i + 1] = rp[i] + (edges.ContainsKey(i) ? edges[i].Count : 0);
            }
            long m = rp[n];
            d = new int[m]; et = new byte[m]; w = new double[m];
            long e = 0;
            for (int i = 0; i < n; i++) {
                if (!edges.ContainsKey(i)) continue;
                foreach (ForwardLink l in edges[i]) { d[e] = l.targetNode; et[e] = (byte)l.type; w[e] = l.weight; e++; }
            }
        }

        bool SameTopology(long[] id, byte[] type, long[] oldRowptr, int[] oldDst) {
            if (oldRowptr == null || oldRowptr.Length != rowptr.Length || oldDst.Length != dst.Length) return false;
            for (int i = 0; i < rowptr.Length; i++) if (oldRowptr[i] != rowptr[i]) return false;
            for (long p = 0; p < dst.LongLength; p++) if (oldDst[p] != dst[p]) return false;
            for (int i = 0; i < id.Length; i++) if (sentId[i] != id[i] || sentType[i] != type[i]) return false;
            return true;
        }

        bool GrownLists(long[] id, byte[] type, long[] oldRowptr, int[] oldDst, byte[] oldEtype, double[] w) {
            if (oldRowptr == null || oldRowptr.Length != rowptr.Length || sentId.Length != id.Length) return false;
            for (int i = 0; i < id.Length; i++) if (sentId[i] != id[i] || sentType[i] != type[i]) return false;
            for (int i = 0; i + 1 < rowptr.Length; i++) {
                long len = oldRowptr[i + 1] - oldRowptr[i];
                if (rowptr[i + 1] - rowptr[i] < len) return false;
                for (long k = 0; k < len; k++) {
                    long o = oldRowptr[i] + k, f = rowptr[i] + k;
                    if (dst[f] != oldDst[o] || etype[f] != oldEtype[o] ||
                        System.BitConverter.DoubleToInt64Bits(w[f]) != System.BitConverter.DoubleToInt64Bits(sentW[o])) return false;
                }
            }
            return true;
        }

        // the node dictionary enumerates its keys as 0, 1, ..., n-1 (what a loader that only ever adds nodes leaves)
        bool KeysInOrder() {
            int k = 0;
            foreach (int key in nodes.Keys) if (key != k++) return false;
            return true;
        }

        // nodes were added behind the last recorded one, the recorded nodes are unchanged, and every recorded list is a bitwise
        // prefix of the new one (the lists of the new nodes count as empty before)
        bool GrownNodes(long[] id, byte[] type, long[] oldRowptr, int[] oldDst, byte[] oldEtype, double[] w) {
            if (oldRowptr == null || sentId.Length >= id.Length) return false;
            int nOld = sentId.Length;
            for (int i = 0; i < nOld; i++) if (sentId[i] != id[i] || sentType[i] != type[i]) return false;
            for (int i = 0; i < nOld; i++) {
                long len = oldRowptr[i + 1] - oldRowptr[i];
                if (rowptr[i + 1] - rowptr[i] < len) return false;
                for (long k = 0; k < len; k++) {
                    long o = oldRowptr[i] + k, f = rowptr[i] + k;
                    if (dst[f] != oldDst[o] || etype[f] != oldEtype[o] ||
                        System.BitConverter.DoubleToInt64Bits(w[f]) != System.BitConverter.DoubleToInt64Bits(sentW[o])) return false;
                }
            }
            return true;
        }

        // fills the public field `graph` (Graph.cs:43) from the device: normalised explicit links per node, null for
        // dangling nodes (Graph.cs:53,64,86)
        public void LoadNormalizedGraph() {
            int n = nodes.Count;
            var wn = new double[System.Math.Max(1, dst.Length)]; var dg = new byte[n];
            Native.Check(Native.rwr_graph_get_normalized(handle, wn, dg));
            var normalized = new Dictionary<int, ForwardLink[]>();
            for (int i = 0; i < n; i++) {
                if (dg[i] != 0) { normalized.Add(i, null); continue; }
                var list = new List<ForwardLink>();
                for (long p = rowptr[i]; p < rowptr[i + 1]; p++)
                    if (etype[p] != 0) list.Add(new ForwardLink(dst[p], (EdgeType)etype[p], wn[p]));
                normalized.Add(i, list.ToArray());
            }
            graph = normalized;
        }

        // addition: the library's counters for this graph (rwr_get_stats), e.g. which kernels served the single-seed SpMV steps
        public RwrStats Stats() {
            var st = new RwrStats { struct_size = System.Runtime.InteropServices.Marshal.SizeOf(typeof(RwrStats)) };
            Native.Check(Native.rwr_get_stats(handle, ref st));
            return st;
        }
        public void ResetStats() { Native.Check(Native.rwr_reset_stats(handle)); }

        public int size() { return nodes.Count; }
    }
}
