// Drop-in replacement of Recommenders/RWRBased/Model.cs: same public fields and methods; run*() execute on
// the GPU through rwr_model_run and leave the result in `rank` exactly as the reference does; deliverRanks() is one
// propagation on the GPU (rwr_model_deliver), updateRanks()/checkConvergence() are the reference's array loops.
// A host-edited `restart` (a public field of the reference, Model.cs:12) takes rwr_model_run_restart /
// rwr_model_deliver_restart instead.  The static RunBatch (an addition) runs many seeds' models in one rwr_model_run_batch call,
// RunRestartBatch many restart vectors' models in one rwr_model_run_restart_batch call.
namespace Recommenders.RWRBased {
    public class Model {
        public Graph graph;
        public double[] rank;
        public double[] nextRank;
        public int nNodes;
        public double dampingFactor;
        public double[] restart;
        int seed = -1;

        public Model(Graph graph, double dampingFactor) {
            this.graph = graph; nNodes = graph.size(); this.dampingFactor = dampingFactor;
            rank = new double[nNodes]; nextRank = new double[nNodes]; restart = new double[nNodes];
            for (int i = 0; i < nNodes; i++) { rank[i] = 1d; restart[i] = 1d / nNodes; }
        }

        public Model(Graph graph, double dampingFactor, int targetNode) {
            this.graph = graph; nNodes = graph.size(); this.dampingFactor = dampingFactor; seed = targetNode;
            rank = new double[nNodes]; nextRank = new double[nNodes]; restart = new double[nNodes];
            for (int i = 0; i < nNodes; i++) { rank[i] = (i == targetNode) ? nNodes : 0; restart[i] = (i == targetNode) ? 1d : 0; }
        }

        // rank / nextRank are still what the constructor left => the whole loop can stay on the device
        bool CtorState() {
            for (int i = 0; i < nNodes; i++) {
                if (nextRank[i] != 0) return false;
                double expect = seed < 0 ? 1d : (i == seed ? nNodes : 0d);
                if (rank[i] != expect) return false;
            }
            return true;
        }

        void Run(int mode, double value) {
            if (CustomRestart()) {
                // the whole loop on the device from the current rank, with the edited restart vector
                for (int i = 0; i < nNodes; i++)
                    if (nextRank[i] != 0)
                        throw new System.InvalidOperationException("run() on a non-zero nextRank: call updateRanks() first");
                long it;
                Native.Check(Native.rwr_model_run_restart(graph.handle, restart, rank, dampingFactor, mode, value, rank, out it));
                return;
            }
            if (CtorState()) {
                long iters;
                Native.Check(Native.rwr_model_run(graph.handle, seed, dampingFactor, mode, value, rank, out iters));
                for (int i = 0; i < nNodes; i++) nextRank[i] = 0;
                return;
            }
            // an already advanced model: the reference's run() continues from the current rank (Model.cs:57-73)
            if (mode == 0) {
                for (int n = 0; n < (int)value; n++) { deliverRanks(); updateRanks(); }
                return;
            }
            double threshold = mode == 2 ? (1 / double.MaxValue) * nNodes : value;
            while (true) {
                deliverRanks();
                if (checkConvergence(threshold)) { updateRanks(); return; }
                updateRanks();
            }
        }
        public void run() { Run(2, 0); }
        public void run(double threshold) { Run(1, threshold); }
        public void run(int nIterations) { Run(0, nIterations); }

        // K personalised models in one call (rwr_model_run_batch), an addition beside the reference surface: ranks[k] and
        // iterations[k] are what new Model(graph, dampingFactor, seeds[k]).run(...) leaves in rank / its step count
        public static double[][] RunBatch(Graph graph, double dampingFactor, int[] seeds, int nIterations, out long[] iterations) {
            return RunBatch(graph, dampingFactor, seeds, 0, nIterations, out iterations);
        }
        public static double[][] RunBatch(Graph graph, double dampingFactor, int[] seeds, double threshold, out long[] iterations) {
            return RunBatch(graph, dampingFactor, seeds, 1, threshold, out iterations);
        }
        public static double[][] RunBatch(Graph graph, double dampingFactor, int[] seeds, out long[] iterations) {
            return RunBatch(graph, dampingFactor, seeds, 2, 0, out iterations);
        }
        static double[][] RunBatch(Graph graph, double dampingFactor, int[] seeds, int mode, double value, out long[] iterations) {
            int K = seeds.Length, n = graph.size();
            var flat = new double[(long)K * n];
            iterations = new long[K];
            Native.Check(Native.rwr_model_run_batch(graph.handle, seeds, K, dampingFactor, mode, value, flat, iterations));
            var ranks = new double[K][];
            for (int k = 0; k < K; k++) {
                ranks[k] = new double[n];
                System.Array.Copy(flat, (long)k * n, ranks[k], 0, n);
            }
            return ranks;
        }

        // K models with caller-set restart vectors in one call (rwr_model_run_restart_batch), an addition beside the reference
        // surface: vector k has restart[nodes[k][j]] = weights[k][j] and zero elsewhere; start[k] >= 0 is the state of
        // new Model(graph, dampingFactor, start[k]), -1 (or start == null) that of new Model(graph, dampingFactor).
        // ranks[k] and iterations[k] are what that Model leaves after its restart field was set and run(...) called
        public static double[][] RunRestartBatch(Graph graph, double dampingFactor, int[][] nodes, double[][] weights,
                                                 int[] start, int nIterations, out long[] iterations) {
            return RunRestartBatch(graph, dampingFactor, nodes, weights, start, 0, nIterations, out iterations);
        }
        public static double[][] RunRestartBatch(Graph graph, double dampingFactor, int[][] nodes, double[][] weights,
                                                 int[] start, double threshold, out long[] iterations) {
            return RunRestartBatch(graph, dampingFactor, nodes, weights, start, 1, threshold, out iterations);
        }
        public static double[][] RunRestartBatch(Graph graph, double dampingFactor, int[][] nodes, double[][] weights,
                                                 int[] start, out long[] iterations) {
            return RunRestartBatch(graph, dampingFactor, nodes, weights, start, 2, 0, out iterations);
        }
        static double[][] RunRestartBatch(Graph graph, double dampingFactor, int[][] nodes, double[][] weights, int[] start,
                                          int mode, double value, out long[] iterations) {
            int K = nodes.Length, n = graph.size();
            if (weights.Length != K || (start != null && start.Length != K))
                throw new System.ArgumentException("nodes, weights and start must hold one entry per vector");
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
            var flat = new double[(long)K * n];
            iterations = new long[K];
            Native.Check(Native.rwr_model_run_restart_batch(graph.handle, K, ptr, idx, val, start, dampingFactor, mode, value, flat,
                                                            iterations));
            var ranks = new double[K][];
            for (int k = 0; k < K; k++) {
                ranks[k] = new double[n];
                System.Array.Copy(flat, (long)k * n, ranks[k], 0, n);
            }
            return ranks;
        }

        // `restart` is a public field of the reference: true when the host has edited it (then the *_restart entry points
        // run; the constructors' one-hot / uniform vectors keep the seed / global paths), as the Python mirror decides
        bool CustomRestart() {
            if (restart == null || restart.Length != nNodes)
                throw new System.ArgumentException("Model.restart must hold nNodes values");
            for (int i = 0; i < nNodes; i++) {
                double expect = seed < 0 ? 1d / nNodes : (i == seed ? 1d : 0d);
                if (restart[i] != expect) return true;
            }
            return false;
        }

        // the reference's public single steps (Model.cs:76,103,110)
        public void deliverRanks() {
            bool custom = CustomRestart();
            for (int i = 0; i < nNodes; i++)
                if (nextRank[i] != 0)
                    throw new System.InvalidOperationException("deliverRanks() on a non-zero nextRank: call updateRanks() first");
            if (custom)
                Native.Check(Native.rwr_model_deliver_restart(graph.handle, restart, dampingFactor, rank, nextRank));
            else
                Native.Check(Native.rwr_model_deliver(graph.handle, seed, dampingFactor, rank, nextRank));
        }
        public void updateRanks() {
            for (int i = 0; i < nNodes; i++) { rank[i] = nextRank[i]; nextRank[i] = 0; }
        }
        public bool checkConvergence(double threshold) {
            double diff = 0;
            for (int i = 0; i < nNodes; i++) diff += System.Math.Abs(rank[i] - nextRank[i]);
            return diff < threshold;
        }
    }
}
