// C++ host mirror of the reference's public surface `namespace Recommenders.RWRBased`
// (Recommenders/RWRBased/{Graph,Model,Recommender}.cs) over the C-ABI of include/rwr.h.
//
// The reference is C# and no C# toolchain exists in the build image, so this header (and the Python mirror
// recommendersystems_amd/rwr_based.py) are the host sides that are actually compiled and exercised; the C# shim
// under csharp/ binds the very same entry points.  Same names, argument meaning and error behaviour as the C#:
//   KeyNotFoundException / ArgumentOutOfRangeException  ->  std::out_of_range
//   any other failure                                   ->  std::runtime_error (with rwr_last_error())
// Header-only; link with librwr.so.
#pragma once
#include <cstdint>
#include <cstring>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../rwr.h"

namespace Recommenders {
namespace RWRBased {

enum class NodeType : uint8_t { UNDEFINED, USER, ITEM, ETC };                                        // Recommender.cs:4
enum class EdgeType : uint8_t { UNDEFINED, LIKE, FRIENDSHIP, FOLLOW, MENTION, AUTHORSHIP, PURCHASE, ETC };  // :5

struct Node {                                                  // Graph.cs:4-17
    int64_t id = 0;
    NodeType type = NodeType::UNDEFINED;
    Node() = default;
    explicit Node(int64_t id_) : id(id_) {}
    Node(int64_t id_, NodeType t) : id(id_), type(t) {}
};

struct ForwardLink {                                           // Graph.cs:19-35 (public mutable fields)
    int targetNode = 0;
    EdgeType type = EdgeType::UNDEFINED;
    double weight = 0;
    ForwardLink() = default;
    ForwardLink(int t, double w) : targetNode(t), weight(w) {}
    ForwardLink(int t, EdgeType ty, double w) : targetNode(t), type(ty), weight(w) {}
};

inline void check(int32_t status)
{
    if (status == RWR_OK) return;
    const std::string msg = rwr_last_error();
    if (status == RWR_E_RANGE) throw std::out_of_range(msg);
    throw std::runtime_error("librwr status " + std::to_string(status) + ": " + msg);
}

class Graph {                                                  // Graph.cs:37-94
public:
    std::map<int, Node> nodes;                                 // Dictionary<int, Node>, keys 0..n-1
    std::map<int, std::vector<ForwardLink>> edges;             // Dictionary<int, List<ForwardLink>>

    Graph(std::map<int, Node> n, std::map<int, std::vector<ForwardLink>> e) : nodes(std::move(n)), edges(std::move(e)) {}
    ~Graph() { rwr_graph_destroy(h_); }
    Graph(const Graph &) = delete;
    Graph &operator=(const Graph &) = delete;

    void buildGraph()                                          // Graph.cs:51-88 -> rwr_graph_create
    {
        const int n = (int)nodes.size();
        std::vector<int64_t> id(n), rowptr(n + 1, 0);
        std::vector<uint8_t> type(n);
        for (int i = 0; i < n; ++i) {
            const Node &nd = nodes.at(i);
            id[i] = nd.id;
            type[i] = (uint8_t)nd.type;
            auto it = edges.find(i);
            rowptr[i + 1] = rowptr[i] + (it == edges.end() ? 0 : (int64_t)it->second.size());
        }
        dst_.assign((size_t)rowptr[n], 0);
        etype_.assign((size_t)rowptr[n], 0);
        std::vector<double> w((size_t)rowptr[n]);
        size_t e = 0;
        for (int i = 0; i < n; ++i) {
            auto it = edges.find(i);
            if (it == edges.end()) continue;
            for (const ForwardLink &l : it->second) { dst_[e] = l.targetNode; etype_[e] = (uint8_t)l.type; w[e] = l.weight; ++e; }
        }
        // buildGraph() again after the host changed link types / weights in place (Experiment.cs:84-101 style): same nodes,
        // list lengths and targets => only the changed links cross the boundary (rwr_graph_update_links)
        if (h_ && id == sent_id_ && type == sent_type_ && rowptr == rowptr_ && dst_ == sent_dst_) {
            std::vector<int64_t> idx;
            std::vector<uint8_t> nt;
            std::vector<double> nw;
            for (size_t p = 0; p < w.size(); ++p)
                if (etype_[p] != sent_etype_[p] || std::memcmp(&w[p], &sent_w_[p], sizeof(double)) != 0) {
                    idx.push_back((int64_t)p); nt.push_back(etype_[p]); nw.push_back(w[p]);
                }
            check(rwr_graph_update_links(h_, (int64_t)idx.size(), idx.data(), nt.data(), nw.data()));
        } else if (h_ && id == sent_id_ && type == sent_type_ && grownLists(rowptr, w)) {
            // same nodes, every old list a bitwise prefix of the new one => only the new links cross (rwr_graph_append_links)
            std::vector<int32_t> as, ad;
            std::vector<uint8_t> at;
            std::vector<double> aw;
            for (int i = 0; i < n; ++i)
                for (int64_t p = rowptr[i] + (rowptr_[i + 1] - rowptr_[i]); p < rowptr[i + 1]; ++p) {
                    as.push_back(i); ad.push_back(dst_[p]); at.push_back(etype_[p]); aw.push_back(w[p]);
                }
            check(rwr_graph_append_links(h_, (int64_t)as.size(), as.data(), ad.data(), at.data(), aw.data(), nullptr));
        } else {
            rwr_graph_destroy(h_);
            h_ = nullptr;
            check(rwr_graph_create(n, id.data(), type.data(), rowptr.data(), dst_.data(), etype_.data(), w.data(), nullptr, &h_));
        }
        rowptr_ = rowptr;
        sent_id_ = id; sent_type_ = type; sent_dst_ = dst_; sent_etype_ = etype_; sent_w_ = w;
    }

    // rwr_graph_append_links on a built graph: link q goes to the end of edges[src[q]] on the device (edges[src].Add(...),
    // Graph.cs:40); returns the positions of the new links in the new flattened raw list.  The caller's `edges` are not
    // touched: add the same links there before the next buildGraph(), which then finds nothing more to send.
    std::vector<int64_t> appendLinks(const std::vector<int32_t> &src, const std::vector<ForwardLink> &links)
    {
        if (src.size() != links.size()) throw std::invalid_argument("one source per link");
        std::vector<int32_t> d(links.size());
        std::vector<uint8_t> t(links.size());
        std::vector<double> w(links.size());
        for (size_t q = 0; q < links.size(); ++q) { d[q] = links[q].targetNode; t[q] = (uint8_t)links[q].type; w[q] = links[q].weight; }
        std::vector<int64_t> pos(links.size());
        check(rwr_graph_append_links(handle(), (int64_t)src.size(), src.data(), d.data(), t.data(), w.data(), pos.data()));
        // the flat copies behind graph() and the next buildGraph()'s diff follow
        const int n = (int)nodes.size();
        std::vector<int64_t> rp(rowptr_);
        std::vector<int64_t> add((size_t)n + 1, 0);
        for (int32_t s : src) ++add[(size_t)s + 1];
        for (int i = 0; i < n; ++i) add[(size_t)i + 1] += add[i];
        for (int i = 0; i <= n; ++i) rp[i] += add[i];
        std::vector<int32_t> nd((size_t)rp[n]);
        std::vector<uint8_t> nt((size_t)rp[n]);
        std::vector<double> nw((size_t)rp[n]);
        for (int i = 0; i < n; ++i)
            for (int64_t p = rowptr_[i]; p < rowptr_[i + 1]; ++p) {
                const size_t f = (size_t)(p + add[i]);
                nd[f] = sent_dst_[p]; nt[f] = sent_etype_[p]; nw[f] = sent_w_[p];
            }
        for (size_t q = 0; q < links.size(); ++q) { nd[(size_t)pos[q]] = d[q]; nt[(size_t)pos[q]] = t[q]; nw[(size_t)pos[q]] = w[q]; }
        rowptr_ = rp; dst_ = nd; etype_ = nt;
        sent_dst_ = nd; sent_etype_ = nt; sent_w_ = nw;
        return pos;
    }

    // rwr_graph_remove_links on a built graph: the raw links at the given flattened positions (distinct, any order) leave
    // their lists on the device (edges[src].RemoveAt(k)); the surviving link at old position e is afterwards at
    // e - (removed positions < e).  The caller's `edges` are not touched: remove the same links there before the next
    // buildGraph(), which then finds nothing more to send.  (Deleting from `edges` WITHOUT this call makes buildGraph() send
    // the graph whole in this binding: only the Python mirror finds removed links by a list diff.)
    void removeLinks(const std::vector<int64_t> &linkIndex)
    {
        check(rwr_graph_remove_links(handle(), (int64_t)linkIndex.size(), linkIndex.data()));
        // the flat copies behind graph() and the next buildGraph()'s diff follow
        const int n = (int)nodes.size();
        std::vector<uint8_t> gone((size_t)rowptr_[n], 0);
        for (int64_t p : linkIndex) gone[(size_t)p] = 1;
        std::vector<int64_t> rp((size_t)n + 1, 0);
        std::vector<int32_t> nd;
        std::vector<uint8_t> nt;
        std::vector<double> nw;
        for (int i = 0; i < n; ++i) {
            for (int64_t p = rowptr_[i]; p < rowptr_[i + 1]; ++p)
                if (!gone[(size_t)p]) { nd.push_back(sent_dst_[p]); nt.push_back(sent_etype_[p]); nw.push_back(sent_w_[p]); }
            rp[(size_t)i + 1] = (int64_t)nd.size();
        }
        rowptr_ = rp; dst_ = nd; etype_ = nt;
        sent_dst_ = nd; sent_etype_ = nt; sent_w_ = nw;
    }

    // rwr_graph_remove_nodes on a built graph: the nodes at the given indices (distinct, any order) leave the graph on the
    // device with every raw link from or to them; the others close up and keep their order.  Returns (newNodeIndex,
    // newLinkIndex): the new index of every old node and the new flattened position of every old link, -1 for what left.
    // The caller's `nodes` / `edges` are not touched: take the same nodes and links out and re-key both by newNodeIndex BEFORE
    // any other call on this object (it reads nodes.size()); the next buildGraph() then finds nothing more to send.
    // (Removing nodes from the maps WITHOUT this call makes buildGraph() send the graph whole in this binding.)
    std::pair<std::vector<int32_t>, std::vector<int64_t>> removeNodes(const std::vector<int32_t> &nodeIndex)
    {
        const size_t n_old = sent_id_.size();
        const size_t m = (size_t)rowptr_[n_old];
        std::vector<int32_t> nn(n_old ? n_old : 1);
        std::vector<int64_t> nl(m ? m : 1);
        int64_t removed = 0;
        check(rwr_graph_remove_nodes(handle(), (int32_t)nodeIndex.size(), nodeIndex.data(), nn.data(), nl.data(), &removed));
        nn.resize(n_old);
        nl.resize(m);
        // the flat copies behind graph() and the next buildGraph()'s diff follow
        const size_t n = n_old - nodeIndex.size();
        std::vector<int64_t> id2(n), rp(n + 1, 0);
        std::vector<uint8_t> ty2(n), nt;
        std::vector<int32_t> nd;
        std::vector<double> nw;
        for (size_t i = 0; i < n_old; ++i) {
            if (nn[i] < 0) continue;
            const size_t to = (size_t)nn[i];
            id2[to] = sent_id_[i]; ty2[to] = sent_type_[i];
            for (int64_t p = rowptr_[i]; p < rowptr_[i + 1]; ++p)
                if (nl[(size_t)p] >= 0) { nd.push_back(nn[(size_t)sent_dst_[p]]); nt.push_back(sent_etype_[p]); nw.push_back(sent_w_[p]); }
            rp[to + 1] = (int64_t)nd.size();
        }
        rowptr_ = rp; dst_ = nd; etype_ = nt;
        sent_id_ = id2; sent_type_ = ty2; sent_dst_ = nd; sent_etype_ = nt; sent_w_ = nw;
        return {nn, nl};
    }

    // the public field Graph.graph (Graph.cs:43): normalised explicit links per node; empty optional == null
    std::map<int, std::unique_ptr<std::vector<ForwardLink>>> graph()
    {
        const int n = (int)nodes.size();
        std::vector<double> wn(dst_.size() ? dst_.size() : 1);
        std::vector<uint8_t> dg(n);
        check(rwr_graph_get_normalized(handle(), wn.data(), dg.data()));
        std::map<int, std::unique_ptr<std::vector<ForwardLink>>> out;
        for (int i = 0; i < n; ++i) {
            if (dg[i]) { out[i] = nullptr; continue; }
            auto v = std::make_unique<std::vector<ForwardLink>>();
            for (int64_t p = rowptr_[i]; p < rowptr_[i + 1]; ++p)
                if (etype_[p] != 0) v->emplace_back(dst_[p], (EdgeType)etype_[p], wn[p]);
            out[i] = std::move(v);
        }
        return out;
    }

    int size() const { return (int)nodes.size(); }             // Graph.cs:91-93
    // addition: the library's counters for this graph (rwr_get_stats) -- among them which kernels served the single-seed SpMV
    // steps (spmv_sweep_launches / spmv_hub_launches / spmv_binned_launches) and the sweep's geometry (sweep_k, sweep_blocks,
    // sweep_wgs, sweep_partial; all 0 when the graph does not take the sweep)
    rwr_stats stats() const
    {
        rwr_stats st{};
        st.struct_size = (int32_t)sizeof(st);
        check(rwr_get_stats(handle(), &st));
        return st;
    }
    void resetStats() { check(rwr_reset_stats(handle())); }
    rwr_graph *handle() const
    {
        if (!h_) throw std::runtime_error("Graph.buildGraph() has not been called");
        return h_;
    }

private:
    // every list as long as before or longer, and its old part bit for bit what the device holds (dst_ / etype_: the new lists)
    bool grownLists(const std::vector<int64_t> &rowptr, const std::vector<double> &w) const
    {
        if (rowptr.size() != rowptr_.size()) return false;
        const size_t n = rowptr.size() - 1;
        for (size_t i = 0; i < n; ++i) {
            const int64_t len = rowptr_[i + 1] - rowptr_[i];
            if (rowptr[i + 1] - rowptr[i] < len) return false;
            for (int64_t k = 0; k < len; ++k) {
                const size_t o = (size_t)(rowptr_[i] + k), f = (size_t)(rowptr[i] + k);
                if (dst_[f] != sent_dst_[o] || etype_[f] != sent_etype_[o] || std::memcmp(&w[f], &sent_w_[o], sizeof(double)) != 0)
                    return false;
            }
        }
        return true;
    }

    rwr_graph *h_ = nullptr;
    std::vector<int64_t> rowptr_;
    std::vector<int32_t> dst_;
    std::vector<uint8_t> etype_;
    // what the device currently holds (for the incremental rebuild)
    std::vector<int64_t> sent_id_;
    std::vector<uint8_t> sent_type_, sent_etype_;
    std::vector<int32_t> sent_dst_;
    std::vector<double> sent_w_;
};

class Model {                                                  // Model.cs:5-116
public:
    Graph &graph;
    std::vector<double> rank, nextRank, restart;
    int nNodes;
    double dampingFactor;

    Model(Graph &g, double d) : graph(g), nNodes(g.size()), dampingFactor(d), seed_(-1)              // :14-31
    {
        rank.assign(nNodes, 1.0);
        nextRank.assign(nNodes, 0.0);
        restart.assign(nNodes, 1.0 / nNodes);
    }
    Model(Graph &g, double d, int targetNode) : graph(g), nNodes(g.size()), dampingFactor(d), seed_(targetNode)   // :33-50
    {
        rank.assign(nNodes, 0.0);
        nextRank.assign(nNodes, 0.0);
        restart.assign(nNodes, 0.0);
        if (targetNode >= 0 && targetNode < nNodes) { rank[targetNode] = nNodes; restart[targetNode] = 1.0; }
    }
    // K personalised models in one call (rwr_model_run_batch), an addition beside the reference surface: ranks[k] /
    // iterations[k] are what Model(g, d, seeds[k]).run(...) leaves in rank / iterations; run(int) / run(double) / run() arguments
    static std::vector<std::vector<double>> runBatch(Graph &g, double d, const std::vector<int> &seeds, int nIterations,
                                                     std::vector<int64_t> *iterations = nullptr)
    { return runBatch_(g, d, seeds, RWR_RUN_ITERATIONS, nIterations, iterations); }
    static std::vector<std::vector<double>> runBatch(Graph &g, double d, const std::vector<int> &seeds, double threshold,
                                                     std::vector<int64_t> *iterations = nullptr)
    { return runBatch_(g, d, seeds, RWR_RUN_THRESHOLD, threshold, iterations); }
    static std::vector<std::vector<double>> runBatch(Graph &g, double d, const std::vector<int> &seeds,
                                                     std::vector<int64_t> *iterations = nullptr)
    { return runBatch_(g, d, seeds, RWR_RUN_DEFAULT_THRESHOLD, 0, iterations); }

    // K models with caller-set restart vectors in one call (rwr_model_run_restart_batch), an addition beside the reference
    // surface: vector k has restart[nodes[k][j]] = weights[k][j] and zero elsewhere; start[k] >= 0 is the state of
    // Model(g, d, start[k]), -1 (or an empty start) that of Model(g, d).  ranks[k] / iterations[k] are what that Model leaves
    // after its restart field was set and run(...) called
    static std::vector<std::vector<double>> runRestartBatch(Graph &g, double d, const std::vector<std::vector<int>> &nodes,
                                                            const std::vector<std::vector<double>> &weights,
                                                            const std::vector<int> &start, int nIterations,
                                                            std::vector<int64_t> *iterations = nullptr)
    { return runRestartBatch_(g, d, nodes, weights, start, RWR_RUN_ITERATIONS, nIterations, iterations); }
    static std::vector<std::vector<double>> runRestartBatch(Graph &g, double d, const std::vector<std::vector<int>> &nodes,
                                                            const std::vector<std::vector<double>> &weights,
                                                            const std::vector<int> &start, double threshold,
                                                            std::vector<int64_t> *iterations = nullptr)
    { return runRestartBatch_(g, d, nodes, weights, start, RWR_RUN_THRESHOLD, threshold, iterations); }
    static std::vector<std::vector<double>> runRestartBatch(Graph &g, double d, const std::vector<std::vector<int>> &nodes,
                                                            const std::vector<std::vector<double>> &weights,
                                                            const std::vector<int> &start,
                                                            std::vector<int64_t> *iterations = nullptr)
    { return runRestartBatch_(g, d, nodes, weights, start, RWR_RUN_DEFAULT_THRESHOLD, 0, iterations); }

    void run() { run_(RWR_RUN_DEFAULT_THRESHOLD, 0); }         // :52-55
    void run(double threshold) { run_(RWR_RUN_THRESHOLD, threshold); }   // :57-66
    void run(int nIterations) { run_(RWR_RUN_ITERATIONS, nIterations); } // :68-73
    int64_t iterations = 0;

    // the reference's public single steps
    void deliverRanks()                                        // :76-100 -> rwr_model_deliver(_restart)
    {
        const bool custom = custom_restart_();
        for (double v : nextRank)
            if (v != 0.0) throw std::logic_error("deliverRanks() on a non-zero nextRank: call updateRanks() first");
        if (custom) check(rwr_model_deliver_restart(graph.handle(), restart.data(), dampingFactor, rank.data(), nextRank.data()));
        else check(rwr_model_deliver(graph.handle(), seed_, dampingFactor, rank.data(), nextRank.data()));
    }
    void updateRanks()                                         // :103-108
    {
        for (int i = 0; i < nNodes; ++i) { rank[i] = nextRank[i]; nextRank[i] = 0.0; }
    }
    bool checkConvergence(double threshold) const              // :110-115
    {
        double diff = 0.0;
        for (int i = 0; i < nNodes; ++i) diff += rank[i] > nextRank[i] ? rank[i] - nextRank[i] : nextRank[i] - rank[i];
        return diff < threshold;
    }

private:
    int seed_;
    static std::vector<std::vector<double>> runBatch_(Graph &g, double d, const std::vector<int> &seeds, int run_mode,
                                                      double value, std::vector<int64_t> *iterations)
    {
        const int32_t K = (int32_t)seeds.size();
        const size_t n = (size_t)g.size();
        std::vector<double> flat((size_t)K * n);
        std::vector<int64_t> it((size_t)K);
        check(rwr_model_run_batch(g.handle(), seeds.data(), K, d, run_mode, value, flat.data(), it.data()));
        std::vector<std::vector<double>> ranks((size_t)K);
        for (int32_t k = 0; k < K; ++k) ranks[k].assign(flat.begin() + (ptrdiff_t)(k * n), flat.begin() + (ptrdiff_t)((k + 1) * n));
        if (iterations) *iterations = it;
        return ranks;
    }
    static std::vector<std::vector<double>> runRestartBatch_(Graph &g, double d, const std::vector<std::vector<int>> &nodes,
                                                             const std::vector<std::vector<double>> &weights,
                                                             const std::vector<int> &start, int run_mode, double value,
                                                             std::vector<int64_t> *iterations)
    {
        const int32_t K = (int32_t)nodes.size();
        const size_t n = (size_t)g.size();
        if (weights.size() != nodes.size() || (!start.empty() && start.size() != nodes.size()))
            throw std::invalid_argument("runRestartBatch: nodes, weights and start must hold one entry per vector");
        std::vector<int64_t> ptr((size_t)K + 1, 0);
        std::vector<int32_t> idx;
        std::vector<double> val;
        for (int32_t k = 0; k < K; ++k) {
            if (nodes[k].size() != weights[k].size())
                throw std::invalid_argument("runRestartBatch: a restart vector's nodes and weights differ in length");
            idx.insert(idx.end(), nodes[k].begin(), nodes[k].end());
            val.insert(val.end(), weights[k].begin(), weights[k].end());
            ptr[(size_t)k + 1] = (int64_t)idx.size();
        }
        std::vector<int32_t> st(start.begin(), start.end());
        std::vector<double> flat((size_t)K * n);
        std::vector<int64_t> it((size_t)K);
        check(rwr_model_run_restart_batch(g.handle(), K, ptr.data(), idx.data(), val.data(), st.empty() ? nullptr : st.data(), d,
                                          run_mode, value, flat.data(), it.data()));
        std::vector<std::vector<double>> ranks((size_t)K);
        for (int32_t k = 0; k < K; ++k) ranks[k].assign(flat.begin() + (ptrdiff_t)(k * n), flat.begin() + (ptrdiff_t)((k + 1) * n));
        if (iterations) *iterations = it;
        return ranks;
    }
    bool ctor_state_() const
    {
        for (int i = 0; i < nNodes; ++i) {
            if (nextRank[i] != 0.0) return false;
            const double expect = seed_ < 0 ? 1.0 : (i == seed_ ? (double)nNodes : 0.0);
            if (rank[i] != expect) return false;
        }
        return true;
    }
    // the public field restart (Model.cs:12) edited by the host: the *_restart entry points serve it
    bool custom_restart_() const
    {
        if ((int)restart.size() != nNodes) throw std::invalid_argument("Model.restart must hold nNodes values");
        for (int i = 0; i < nNodes; ++i) {
            const double expect = seed_ < 0 ? 1.0 / nNodes : (i == seed_ ? 1.0 : 0.0);
            if (restart[i] != expect) return true;
        }
        return false;
    }
    void run_(int mode, double value)
    {
        if (custom_restart_()) {                               // the whole loop on the device, from the current rank
            for (double v : nextRank)
                if (v != 0.0) throw std::logic_error("run() on a non-zero nextRank: call updateRanks() first");
            check(rwr_model_run_restart(graph.handle(), restart.data(), rank.data(), dampingFactor, mode, value, rank.data(),
                                        &iterations));
            return;
        }
        if (ctor_state_()) {                                   // the whole loop stays on the device
            check(rwr_model_run(graph.handle(), seed_, dampingFactor, mode, value, rank.data(), &iterations));
            nextRank.assign(nNodes, 0.0);
            return;
        }
        // an already advanced model: the reference's run() continues from the current rank (Model.cs:57-73)
        iterations = 0;
        if (mode == RWR_RUN_ITERATIONS) {
            for (int64_t k = 0; k < (int64_t)value; ++k) { deliverRanks(); updateRanks(); ++iterations; }
            return;
        }
        const double threshold = mode == RWR_RUN_DEFAULT_THRESHOLD ? (1 / 1.7976931348623157e308) * nNodes : value;
        for (;;) {
            deliverRanks();
            ++iterations;
            const bool done = checkConvergence(threshold);
            updateRanks();
            if (done) return;
        }
    }
};

class Recommender {                                            // Recommender.cs:7-52
public:
    explicit Recommender(Graph &g) : graph_(g) {}

    std::vector<std::pair<int64_t, double>> Recommendation(int idxTargetUser, float dampingFactor, int nIteration,
                                                           int topN = 0)                     // :14-40, :42-51
    {
        if (!graph_.edges.count(idxTargetUser)) throw std::out_of_range("KeyNotFound: graph.edges[idxTargetUser]");   // :21
        int64_t count = graph_.size();
        std::vector<int64_t> ids((size_t)count);
        std::vector<double> scores((size_t)count);
        check(rwr_recommend(graph_.handle(), idxTargetUser, dampingFactor, nIteration, topN, ids.data(), scores.data(),
                            &count));
        std::vector<std::pair<int64_t, double>> out((size_t)count);
        for (int64_t i = 0; i < count; ++i) out[i] = {ids[i], scores[i]};
        return out;
    }

    // addition: the top-N lists of K seeds among the nodes of ONE node type (rwr_recommend_typed_batch).  candType: the
    // candidates' type; exclEdgeTypes: the targets of the seed's raw links of these types are no candidates; excludeSelf: neither
    // is the seed.  "Who to follow" is (NodeType::USER, {FRIENDSHIP, FOLLOW}, true)
    std::vector<std::vector<std::pair<int64_t, double>>> recommendTypedBatch(const std::vector<int> &seeds, float dampingFactor,
                                                                             int nIteration, int topN, NodeType candType,
                                                                             const std::vector<EdgeType> &exclEdgeTypes = {},
                                                                             bool excludeSelf = false)
    {
        const int32_t K = (int32_t)seeds.size();
        if (topN < 1) throw std::invalid_argument("recommendTypedBatch: topN must be >= 1");
        uint32_t mask = 0;
        for (EdgeType t : exclEdgeTypes) mask |= 1u << (unsigned)t;
        std::vector<int32_t> sd(seeds.begin(), seeds.end());
        std::vector<int64_t> ids((size_t)K * (size_t)topN);
        std::vector<double> scores((size_t)K * (size_t)topN);
        std::vector<int32_t> counts((size_t)K);
        check(rwr_recommend_typed_batch(graph_.handle(), sd.data(), K, dampingFactor, nIteration, topN, (int32_t)candType, mask, excludeSelf ? 1 : 0, ids.data(), scores.data(), counts.data()));
        std::vector<std::vector<std::pair<int64_t, double>>> out((size_t)K);
        for (int32_t k = 0; k < K; ++k)
            for (int32_t q = 0; q < counts[k]; ++q)
                out[k].emplace_back(ids[(size_t)k * (size_t)topN + q], scores[(size_t)k * (size_t)topN + q]);
        return out;
    }

    // addition: the audiences of K targets (rwr_recommend_audience_batch) -- list k ranks the nodes s of candType (< 0: of any
    // type) by the score a walk of nIteration steps FROM s gives targets[k], by one reverse walk per target.  The nodes with a
    // raw link of a type in exclEdgeTypes to targets[k] are left out, targets[k] itself too with excludeSelf.  The scores
    // agree with the forward walks' to the tolerance rwr.h derives, not bitwise.  nodes (may be nullptr) receives the
    // entries' node indices, list by list
    std::vector<std::vector<std::pair<int64_t, double>>> audienceBatch(const std::vector<int> &targets, float dampingFactor,
                                                                       int nIteration, int candType,
                                                                       const std::vector<EdgeType> &exclEdgeTypes = {},
                                                                       bool excludeSelf = false, int topN = 100,
                                                                       std::vector<std::vector<int32_t>> *nodes = nullptr)
    {
        const int32_t K = (int32_t)targets.size();
        if (topN < 1) throw std::invalid_argument("audienceBatch: topN must be >= 1");
        uint32_t mask = 0;
        for (EdgeType t : exclEdgeTypes) mask |= 1u << (unsigned)t;
        std::vector<int32_t> tg(targets.begin(), targets.end());
        std::vector<int64_t> ids((size_t)K * (size_t)topN);
        std::vector<double> scores((size_t)K * (size_t)topN);
        std::vector<int32_t> rows((size_t)K * (size_t)topN), counts((size_t)K);
        check(rwr_recommend_audience_batch(graph_.handle(), K, tg.data(), dampingFactor, nIteration, candType < 0 ? -1 : candType, mask, excludeSelf ? 1 : 0, topN, ids.data(), scores.data(), rows.data(), counts.data()));
        std::vector<std::vector<std::pair<int64_t, double>>> out((size_t)K);
        if (nodes) nodes->assign((size_t)K, {});
        for (int32_t k = 0; k < K; ++k)
            for (int32_t q = 0; q < counts[k]; ++q) {
                out[k].emplace_back(ids[(size_t)k * (size_t)topN + q], scores[(size_t)k * (size_t)topN + q]);
                if (nodes) (*nodes)[k].push_back(rows[(size_t)k * (size_t)topN + q]);
            }
        return out;
    }

    // addition: the audiences of K weighted target SETS (rwr_recommend_audience_set_batch) -- list k ranks the nodes s of candType
    // (< 0: of any type) by sum_v weights[k][v] * (the score a walk FROM s gives member v of sets[k]).  weights == nullptr: 1.0
    // each, else one weight per member; a member that repeats has its weights added.  Left out: the nodes with a raw link of a
    // type in exclEdgeTypes to any member, the members with excludeMembers, the node indices of (*deny)[k], and with a pool
    // (node indices, any order) every node outside it.  nodes (may be nullptr) receives the entries' node indices
    std::vector<std::vector<std::pair<int64_t, double>>> audienceSetBatch(const std::vector<std::vector<int>> &sets, float dampingFactor,
                                                                          int nIteration,
                                                                          const std::vector<std::vector<double>> *weights = nullptr,
                                                                          int candType = -1,
                                                                          const std::vector<EdgeType> &exclEdgeTypes = {},
                                                                          bool excludeMembers = false,
                                                                          const std::vector<int> *pool = nullptr,
                                                                          const std::vector<std::vector<int>> *deny = nullptr,
                                                                          int topN = 100,
                                                                          std::vector<std::vector<int32_t>> *nodes = nullptr)
    {
        if (topN < 1) throw std::invalid_argument("audienceSetBatch: topN must be >= 1");
        AudienceSets a = packAudienceSets_(sets, weights, exclEdgeTypes, pool, deny);
        const int32_t K = a.K;
        std::vector<int64_t> ids((size_t)K * (size_t)topN);
        std::vector<double> scores((size_t)K * (size_t)topN);
        std::vector<int32_t> rows((size_t)K * (size_t)topN), counts((size_t)K);
        check(rwr_recommend_audience_set_batch(graph_.handle(), K, a.sp.data(), a.si.data(), weights ? a.sw.data() : nullptr, dampingFactor, nIteration, candType < 0 ? -1 : candType, a.mask, excludeMembers ? 1 : 0, a.nPool, a.pool.data(), deny ? a.dp.data() : nullptr, a.di.data(), topN, ids.data(), scores.data(), rows.data(), counts.data()));
        std::vector<std::vector<std::pair<int64_t, double>>> out((size_t)K);
        if (nodes) nodes->assign((size_t)K, {});
        for (int32_t k = 0; k < K; ++k)
            for (int32_t q = 0; q < counts[k]; ++q) {
                out[k].emplace_back(ids[(size_t)k * (size_t)topN + q], scores[(size_t)k * (size_t)topN + q]);
                if (nodes) (*nodes)[k].push_back(rows[(size_t)k * (size_t)topN + q]);
            }
        return out;
    }

    // ... for one set
    std::vector<std::pair<int64_t, double>> audienceSet(const std::vector<int> &members, float dampingFactor, int nIteration,
                                                        const std::vector<double> *weights = nullptr, int candType = -1,
                                                        const std::vector<EdgeType> &exclEdgeTypes = {}, bool excludeMembers = false,
                                                        const std::vector<int> *pool = nullptr, const std::vector<int> *deny = nullptr,
                                                        int topN = 100)
    {
        const std::vector<std::vector<double>> w1 = {weights ? *weights : std::vector<double>()};
        const std::vector<std::vector<int>> d1 = {deny ? *deny : std::vector<int>()};
        return audienceSetBatch({members}, dampingFactor, nIteration, weights ? &w1 : nullptr, candType, exclEdgeTypes, excludeMembers,
                                pool, deny ? &d1 : nullptr, topN)[0];
    }

    // addition: audienceSetBatch for lists of up to RWR_LONG_TOP_N_MAX = 65 536 entries (rwr_recommend_audience_set_long_batch): up
    // to 1 024 entries it returns audienceSetBatch's lists, a longer list continues them.  The arguments as there
    std::vector<std::vector<std::pair<int64_t, double>>> audienceSetLongBatch(const std::vector<std::vector<int>> &sets, float dampingFactor,
                                                                              int nIteration,
                                                                              const std::vector<std::vector<double>> *weights = nullptr,
                                                                              int candType = -1,
                                                                              const std::vector<EdgeType> &exclEdgeTypes = {},
                                                                              bool excludeMembers = false,
                                                                              const std::vector<int> *pool = nullptr,
                                                                              const std::vector<std::vector<int>> *deny = nullptr,
                                                                              int topN = 4096,
                                                                              std::vector<std::vector<int32_t>> *nodes = nullptr)
    {
        if (topN < 1) throw std::invalid_argument("audienceSetLongBatch: topN must be >= 1");
        AudienceSets a = packAudienceSets_(sets, weights, exclEdgeTypes, pool, deny);
        const int32_t K = a.K;
        std::vector<int64_t> ids((size_t)K * (size_t)topN);
        std::vector<double> scores((size_t)K * (size_t)topN);
        std::vector<int32_t> rows((size_t)K * (size_t)topN), counts((size_t)K);
        check(rwr_recommend_audience_set_long_batch(graph_.handle(), K, a.sp.data(), a.si.data(), weights ? a.sw.data() : nullptr, dampingFactor, nIteration, candType < 0 ? -1 : candType, a.mask, excludeMembers ? 1 : 0, a.nPool, a.pool.data(), deny ? a.dp.data() : nullptr, a.di.data(), topN, ids.data(), scores.data(), rows.data(), counts.data()));
        std::vector<std::vector<std::pair<int64_t, double>>> out((size_t)K);
        if (nodes) nodes->assign((size_t)K, {});
        for (int32_t k = 0; k < K; ++k)
            for (int32_t q = 0; q < counts[k]; ++q) {
                out[k].emplace_back(ids[(size_t)k * (size_t)topN + q], scores[(size_t)k * (size_t)topN + q]);
                if (nodes) (*nodes)[k].push_back(rows[(size_t)k * (size_t)topN + q]);
            }
        return out;
    }

    // ... for one set
    std::vector<std::pair<int64_t, double>> audienceSetLong(const std::vector<int> &members, float dampingFactor, int nIteration,
                                                            const std::vector<double> *weights = nullptr, int candType = -1,
                                                            const std::vector<EdgeType> &exclEdgeTypes = {}, bool excludeMembers = false,
                                                            const std::vector<int> *pool = nullptr, const std::vector<int> *deny = nullptr,
                                                            int topN = 4096)
    {
        const std::vector<std::vector<double>> w1 = {weights ? *weights : std::vector<double>()};
        const std::vector<std::vector<int>> d1 = {deny ? *deny : std::vector<int>()};
        return audienceSetLongBatch({members}, dampingFactor, nIteration, weights ? &w1 : nullptr, candType, exclEdgeTypes, excludeMembers,
                                    pool, deny ? &d1 : nullptr, topN)[0];
    }

    // ... and the 0-based position and score of every test id in the sets' WHOLE audience lists
    // (rwr_recommend_audience_set_positions_batch): positions[k][j] / scores[k][j] answer testSets[k][j] (-1 / +0.0: not in the
    // list), listLen[k] is list k's length.  scores and listLen may be nullptr
    std::vector<std::vector<int64_t>> audienceSetPositionsBatch(const std::vector<std::vector<int>> &sets, float dampingFactor,
                                                                int nIteration, const std::vector<std::vector<int64_t>> &testSets,
                                                                const std::vector<std::vector<double>> *weights = nullptr,
                                                                int candType = -1, const std::vector<EdgeType> &exclEdgeTypes = {},
                                                                bool excludeMembers = false, const std::vector<int> *pool = nullptr,
                                                                const std::vector<std::vector<int>> *deny = nullptr,
                                                                std::vector<std::vector<double>> *scores = nullptr,
                                                                std::vector<int64_t> *listLen = nullptr)
    {
        AudienceSets a = packAudienceSets_(sets, weights, exclEdgeTypes, pool, deny);
        const int32_t K = a.K;
        if ((int32_t)testSets.size() != K) throw std::invalid_argument("audienceSetPositionsBatch: one test set per target set");
        std::vector<int64_t> tp((size_t)K + 1, 0), ti;
        for (int32_t k = 0; k < K; ++k) {
            ti.insert(ti.end(), testSets[k].begin(), testSets[k].end());
            tp[(size_t)k + 1] = (int64_t)ti.size();
        }
        std::vector<int64_t> pos(ti.size() + 1, -1), len((size_t)K + 1, 0);
        std::vector<double> sc(ti.size() + 1, 0.0);
        ti.push_back(0);
        check(rwr_recommend_audience_set_positions_batch(graph_.handle(), K, a.sp.data(), a.si.data(), weights ? a.sw.data() : nullptr, dampingFactor, nIteration, candType < 0 ? -1 : candType, a.mask, excludeMembers ? 1 : 0, a.nPool, a.pool.data(), deny ? a.dp.data() : nullptr, a.di.data(), tp.data(), ti.data(), pos.data(), sc.data(), len.data()));
        std::vector<std::vector<int64_t>> out((size_t)K);
        if (scores) scores->assign((size_t)K, {});
        for (int32_t k = 0; k < K; ++k) {
            out[k].assign(pos.begin() + tp[(size_t)k], pos.begin() + tp[(size_t)k + 1]);
            if (scores) (*scores)[k].assign(sc.begin() + tp[(size_t)k], sc.begin() + tp[(size_t)k + 1]);
        }
        if (listLen) listLen->assign(len.begin(), len.begin() + K);
        return out;
    }

    // addition: the same lists within a candidate pool, with a deny list per seed and with a diversity cap -- at most groupCap
    // entries per group of nodes in every list (rwr_recommend_capped_batch).  candType < 0: nodes of any type; pool == nullptr:
    // no pool, else node INDICES in any order; deny == nullptr: no deny lists, else one list of node indices per seed; groupOf
    // == nullptr: no cap, else one label per node of the graph (a negative label: never capped); groupCap in [1, 8].
    // Candidates the mask, excludeSelf, the pool or a deny list remove do not use up a group's allowance
    std::vector<std::vector<std::pair<int64_t, double>>> recommendCappedBatch(const std::vector<int> &seeds, float dampingFactor,
                                                                              int nIteration, int topN, int candType,
                                                                              const std::vector<EdgeType> &exclEdgeTypes,
                                                                              bool excludeSelf, const std::vector<int32_t> *pool,
                                                                              const std::vector<std::vector<int32_t>> *deny,
                                                                              const std::vector<int32_t> *groupOf, int groupCap)
    {
        const int32_t K = (int32_t)seeds.size();
        if (topN < 1) throw std::invalid_argument("recommendCappedBatch: topN must be >= 1");
        if (deny && deny->size() != seeds.size()) throw std::invalid_argument("recommendCappedBatch: deny must hold one entry per seed");
        uint32_t mask = 0;
        for (EdgeType t : exclEdgeTypes) mask |= 1u << (unsigned)t;
        std::vector<int32_t> sd(seeds.begin(), seeds.end());
        std::vector<int64_t> dptr((size_t)K + 1, 0);
        std::vector<int32_t> didx;
        if (deny)
            for (int32_t k = 0; k < K; ++k) {
                didx.insert(didx.end(), (*deny)[(size_t)k].begin(), (*deny)[(size_t)k].end());
                dptr[(size_t)k + 1] = (int64_t)didx.size();
            }
        didx.push_back(0);                                       // (at least one element behind the pointer)
        const int32_t none = 0;
        std::vector<int64_t> ids((size_t)K * (size_t)topN);
        std::vector<double> scores((size_t)K * (size_t)topN);
        std::vector<int32_t> counts((size_t)K);
        check(rwr_recommend_capped_batch(graph_.handle(), sd.data(), K, dampingFactor, nIteration, topN, candType < 0 ? -1 : candType, mask, excludeSelf ? 1 : 0, pool ? (int64_t)pool->size() : -1, pool ? (pool->empty() ? &none : pool->data()) : nullptr, deny ? dptr.data() : nullptr, deny ? didx.data() : nullptr, groupOf ? groupOf->data() : nullptr, groupCap, ids.data(), scores.data(), counts.data()));
        std::vector<std::vector<std::pair<int64_t, double>>> out((size_t)K);
        for (int32_t k = 0; k < K; ++k)
            for (int32_t q = 0; q < counts[k]; ++q)
                out[k].emplace_back(ids[(size_t)k * (size_t)topN + q], scores[(size_t)k * (size_t)topN + q]);
        return out;
    }

    // addition: recommendCappedBatch for lists of up to RWR_LONG_TOP_N_MAX = 65 536 entries (rwr_recommend_long_batch): candidates
    // for a re-ranker.  The order is score descending, id descending, node index ascending; nodes (may be nullptr) receives the
    // entries' node indices.  Up to 1 024 entries the call is recommendExplainedBatch without reasons.  The other arguments as in
    // recommendCappedBatch
    std::vector<std::vector<std::pair<int64_t, double>>> recommendLongBatch(const std::vector<int> &seeds, float dampingFactor,
                                                                            int nIteration, int topN, int candType,
                                                                            const std::vector<EdgeType> &exclEdgeTypes,
                                                                            bool excludeSelf, const std::vector<int32_t> *pool,
                                                                            const std::vector<std::vector<int32_t>> *deny,
                                                                            const std::vector<int32_t> *groupOf, int groupCap,
                                                                            std::vector<std::vector<int32_t>> *nodes = nullptr)
    {
        const int32_t K = (int32_t)seeds.size();
        if (topN < 1 || topN > RWR_LONG_TOP_N_MAX) throw std::invalid_argument("recommendLongBatch: topN must lie in [1, 65536]");
        if (deny && deny->size() != seeds.size()) throw std::invalid_argument("recommendLongBatch: deny must hold one entry per seed");
        uint32_t mask = 0;
        for (EdgeType t : exclEdgeTypes) mask |= 1u << (unsigned)t;
        std::vector<int32_t> sd(seeds.begin(), seeds.end());
        std::vector<int64_t> dptr((size_t)K + 1, 0);
        std::vector<int32_t> didx;
        if (deny)
            for (int32_t k = 0; k < K; ++k) {
                didx.insert(didx.end(), (*deny)[(size_t)k].begin(), (*deny)[(size_t)k].end());
                dptr[(size_t)k + 1] = (int64_t)didx.size();
            }
        didx.push_back(0);                                       // (at least one element behind the pointer)
        const int32_t none = 0;
        std::vector<int64_t> ids((size_t)K * (size_t)topN);
        std::vector<double> scores((size_t)K * (size_t)topN);
        std::vector<int32_t> counts((size_t)K), rows(nodes ? (size_t)K * (size_t)topN : 0);
        check(rwr_recommend_long_batch(graph_.handle(), sd.data(), K, dampingFactor, nIteration, topN, candType < 0 ? -1 : candType, mask, excludeSelf ? 1 : 0, pool ? (int64_t)pool->size() : -1, pool ? (pool->empty() ? &none : pool->data()) : nullptr, deny ? dptr.data() : nullptr, deny ? didx.data() : nullptr, groupOf ? groupOf->data() : nullptr, groupCap, ids.data(), scores.data(), counts.data(), nodes ? rows.data() : nullptr));
        std::vector<std::vector<std::pair<int64_t, double>>> out((size_t)K);
        if (nodes) nodes->assign((size_t)K, {});
        for (int32_t k = 0; k < K; ++k)
            for (int32_t q = 0; q < counts[k]; ++q) {
                out[k].emplace_back(ids[(size_t)k * (size_t)topN + q], scores[(size_t)k * (size_t)topN + q]);
                if (nodes) (*nodes)[k].push_back(rows[(size_t)k * (size_t)topN + q]);
            }
        return out;
    }

    // ... for one seed (deny: its one deny list)
    std::vector<std::pair<int64_t, double>> recommendLong(int idxTargetNode, float dampingFactor, int nIteration, int topN, int candType,
                                                          const std::vector<EdgeType> &exclEdgeTypes = {}, bool excludeSelf = false,
                                                          const std::vector<int32_t> *pool = nullptr, const std::vector<int32_t> *deny = nullptr,
                                                          const std::vector<int32_t> *groupOf = nullptr, int groupCap = 1)
    {
        const std::vector<std::vector<int32_t>> d1 = {deny ? *deny : std::vector<int32_t>()};
        return recommendLongBatch({idxTargetNode}, dampingFactor, nIteration, topN, candType, exclEdgeTypes, excludeSelf, pool,
                                  deny ? &d1 : nullptr, groupOf, groupCap)[0];
    }

    // addition: recommendCappedBatch with the reasons of every list entry (rwr_recommend_explained_batch): per entry its node
    // index, the source node and the value of its nWhy (0 to 8) largest in-link addends fl(fl((1 - d) * previousRank[u]) *
    // weight(u -> v)), largest first (-1 / +0.0 where fewer are positive), and the number of positive addends.  All tables are
    // K x topN (x nWhy) row-major, cells behind a list's end hold -1 / -1 / +0.0 / 0.  The other arguments as in
    // recommendCappedBatch
    struct Explained {
        std::vector<int64_t> ids;
        std::vector<double> scores;
        std::vector<int32_t> counts, nodes, whySrc;
        std::vector<double> whyTerm;
        std::vector<int64_t> whyTotal;
    };
    Explained recommendExplainedBatch(const std::vector<int> &seeds, float dampingFactor, int nIteration, int topN, int nWhy, int candType,
                                      const std::vector<EdgeType> &exclEdgeTypes, bool excludeSelf, const std::vector<int32_t> *pool,
                                      const std::vector<std::vector<int32_t>> *deny, const std::vector<int32_t> *groupOf, int groupCap)
    {
        const int32_t K = (int32_t)seeds.size();
        if (topN < 1) throw std::invalid_argument("recommendExplainedBatch: topN must be >= 1");
        if (nWhy < 0 || nWhy > RWR_WHY_MAX) throw std::invalid_argument("recommendExplainedBatch: nWhy must lie in [0, 8]");
        if (deny && deny->size() != seeds.size()) throw std::invalid_argument("recommendExplainedBatch: deny must hold one entry per seed");
        uint32_t mask = 0;
        for (EdgeType t : exclEdgeTypes) mask |= 1u << (unsigned)t;
        std::vector<int32_t> sd(seeds.begin(), seeds.end());
        std::vector<int64_t> dptr((size_t)K + 1, 0);
        std::vector<int32_t> didx;
        if (deny)
            for (int32_t k = 0; k < K; ++k) {
                didx.insert(didx.end(), (*deny)[(size_t)k].begin(), (*deny)[(size_t)k].end());
                dptr[(size_t)k + 1] = (int64_t)didx.size();
            }
        didx.push_back(0);                                       // (at least one element behind the pointer)
        const int32_t none = 0;
        const size_t cells = (size_t)K * (size_t)topN;
        Explained e;
        e.ids.resize(cells), e.scores.resize(cells), e.counts.resize((size_t)K), e.nodes.resize(cells), e.whyTotal.resize(cells);
        e.whySrc.resize(cells * (size_t)nWhy + 1), e.whyTerm.resize(cells * (size_t)nWhy + 1);
        check(rwr_recommend_explained_batch(graph_.handle(), sd.data(), K, dampingFactor, nIteration, topN, candType < 0 ? -1 : candType, mask, excludeSelf ? 1 : 0, pool ? (int64_t)pool->size() : -1, pool ? (pool->empty() ? &none : pool->data()) : nullptr, deny ? dptr.data() : nullptr, deny ? didx.data() : nullptr, groupOf ? groupOf->data() : nullptr, groupCap, nWhy, e.ids.data(), e.scores.data(), e.counts.data(), e.nodes.data(), e.whySrc.data(), e.whyTerm.data(), e.whyTotal.data()));
        e.whySrc.resize(cells * (size_t)nWhy), e.whyTerm.resize(cells * (size_t)nWhy);
        return e;
    }

    // addition: Hits and the running-precision sum (Experiment.cs:121-128) of K seeds' WHOLE lists among the nodes of one node
    // type against one test set each, evaluated on the device without writing a ranked list (rwr_recommend_typed_eval_batch).
    // candType, exclEdgeTypes and excludeSelf as in recommendTypedBatch; topN > 0 evaluates the first topN entries of every
    // list (any value), topN <= 0 the whole list
    struct TypedEval {
        std::vector<int64_t> nHits;
        std::vector<double> sumPrecision;
        std::vector<int64_t> listLen;
    };
    TypedEval recommendTypedEvalBatch(const std::vector<int> &seeds, float dampingFactor, int nIteration,
                                      const std::vector<std::vector<int64_t>> &testSets, NodeType candType,
                                      const std::vector<EdgeType> &exclEdgeTypes = {}, bool excludeSelf = false, int topN = 0)
    {
        const int32_t K = (int32_t)seeds.size();
        if (testSets.size() != seeds.size()) throw std::invalid_argument("recommendTypedEvalBatch: testSets must hold one entry per seed");
        uint32_t mask = 0;
        for (EdgeType t : exclEdgeTypes) mask |= 1u << (unsigned)t;
        std::vector<int32_t> sd(seeds.begin(), seeds.end());
        std::vector<int64_t> tptr((size_t)K + 1, 0), tids;
        for (int32_t k = 0; k < K; ++k) {
            tids.insert(tids.end(), testSets[k].begin(), testSets[k].end());
            tptr[(size_t)k + 1] = (int64_t)tids.size();
        }
        TypedEval out{std::vector<int64_t>((size_t)K), std::vector<double>((size_t)K), std::vector<int64_t>((size_t)K)};
        check(rwr_recommend_typed_eval_batch(graph_.handle(), sd.data(), K, dampingFactor, nIteration, topN, (int32_t)candType, mask, excludeSelf ? 1 : 0, tptr.data(), tids.data(), out.nHits.data(), out.sumPrecision.data(), out.listLen.data()));
        return out;
    }

    // addition: the top-N lists of K walks with caller-set restart vectors among the nodes of ONE node type
    // (rwr_recommend_restart_typed_batch).  nodes / weights / start / exclude as in recommendRestartBatch; candType and
    // exclEdgeTypes as in recommendTypedBatch, applied to every member of exclusion set k; excludeMembers: the members
    // themselves are no candidates.  "Whom should this group follow" is (NodeType::USER, {FRIENDSHIP, FOLLOW}, true)
    std::vector<std::vector<std::pair<int64_t, double>>> recommendRestartTypedBatch(
        const std::vector<std::vector<int>> &nodes, const std::vector<std::vector<double>> &weights, const std::vector<int> &start,
        double dampingFactor, int nIteration, int topN, NodeType candType, const std::vector<EdgeType> &exclEdgeTypes = {},
        bool excludeMembers = false, const std::vector<std::vector<int>> *exclude = nullptr)
    {
        const int32_t K = (int32_t)nodes.size();
        if (topN < 1) throw std::invalid_argument("recommendRestartTypedBatch: topN must be >= 1");
        if (weights.size() != nodes.size() || (!start.empty() && start.size() != nodes.size()) ||
            (exclude && exclude->size() != nodes.size()))
            throw std::invalid_argument("recommendRestartTypedBatch: nodes, weights, start and exclude must hold one entry per vector");
        uint32_t mask = 0;
        for (EdgeType t : exclEdgeTypes) mask |= 1u << (unsigned)t;
        std::vector<int64_t> ptr((size_t)K + 1, 0), eptr((size_t)K + 1, 0);
        std::vector<int32_t> idx, eidx;
        std::vector<double> val;
        for (int32_t k = 0; k < K; ++k) {
            if (nodes[k].size() != weights[k].size())
                throw std::invalid_argument("recommendRestartTypedBatch: a restart vector's nodes and weights differ in length");
            idx.insert(idx.end(), nodes[k].begin(), nodes[k].end());
            val.insert(val.end(), weights[k].begin(), weights[k].end());
            ptr[(size_t)k + 1] = (int64_t)idx.size();
            if (exclude) eidx.insert(eidx.end(), (*exclude)[k].begin(), (*exclude)[k].end());
            eptr[(size_t)k + 1] = (int64_t)eidx.size();
        }
        std::vector<int32_t> st(start.begin(), start.end());
        std::vector<int64_t> ids((size_t)K * (size_t)topN);
        std::vector<double> scores((size_t)K * (size_t)topN);
        std::vector<int32_t> counts((size_t)K);
        check(rwr_recommend_restart_typed_batch(graph_.handle(), K, ptr.data(), idx.data(), val.data(), st.empty() ? nullptr : st.data(), exclude ? eptr.data() : nullptr, eidx.data(), dampingFactor, nIteration, topN, (int32_t)candType, mask, excludeMembers ? 1 : 0, ids.data(), scores.data(), counts.data()));
        std::vector<std::vector<std::pair<int64_t, double>>> out((size_t)K);
        for (int32_t k = 0; k < K; ++k)
            for (int32_t q = 0; q < counts[k]; ++q)
                out[k].emplace_back(ids[(size_t)k * (size_t)topN + q], scores[(size_t)k * (size_t)topN + q]);
        return out;
    }

    // addition: the top-N lists of K walks with caller-set restart vectors, ranked on the device (rwr_recommend_restart_batch).
    // nodes / weights (>= 0) / start as in Model::runRestartBatch.  exclude[k]: the nodes whose LIKEd items are not candidates
    // of vector k (Recommender.cs:20-24 for each of them); exclude == nullptr: the nodes of vector k's own support
    std::vector<std::vector<std::pair<int64_t, double>>> recommendRestartBatch(
        const std::vector<std::vector<int>> &nodes, const std::vector<std::vector<double>> &weights, const std::vector<int> &start,
        double dampingFactor, int nIteration, int topN, const std::vector<std::vector<int>> *exclude = nullptr)
    {
        const int32_t K = (int32_t)nodes.size();
        if (topN < 1) throw std::invalid_argument("recommendRestartBatch: topN must be >= 1");
        if (weights.size() != nodes.size() || (!start.empty() && start.size() != nodes.size()) ||
            (exclude && exclude->size() != nodes.size()))
            throw std::invalid_argument("recommendRestartBatch: nodes, weights, start and exclude must hold one entry per vector");
        std::vector<int64_t> ptr((size_t)K + 1, 0), eptr((size_t)K + 1, 0);
        std::vector<int32_t> idx, eidx;
        std::vector<double> val;
        for (int32_t k = 0; k < K; ++k) {
            if (nodes[k].size() != weights[k].size())
                throw std::invalid_argument("recommendRestartBatch: a restart vector's nodes and weights differ in length");
            idx.insert(idx.end(), nodes[k].begin(), nodes[k].end());
            val.insert(val.end(), weights[k].begin(), weights[k].end());
            ptr[(size_t)k + 1] = (int64_t)idx.size();
            if (exclude) eidx.insert(eidx.end(), (*exclude)[k].begin(), (*exclude)[k].end());
            eptr[(size_t)k + 1] = (int64_t)eidx.size();
        }
        std::vector<int32_t> st(start.begin(), start.end());
        std::vector<int64_t> ids((size_t)K * (size_t)topN);
        std::vector<double> scores((size_t)K * (size_t)topN);
        std::vector<int32_t> counts((size_t)K);
        check(rwr_recommend_restart_batch(graph_.handle(), K, ptr.data(), idx.data(), val.data(), st.empty() ? nullptr : st.data(),
                                          exclude ? eptr.data() : nullptr, eidx.data(), dampingFactor, nIteration, topN,
                                          ids.data(), scores.data(), counts.data()));
        std::vector<std::vector<std::pair<int64_t, double>>> out((size_t)K);
        for (int32_t k = 0; k < K; ++k)
            for (int32_t q = 0; q < counts[k]; ++q)
                out[k].emplace_back(ids[(size_t)k * (size_t)topN + q], scores[(size_t)k * (size_t)topN + q]);
        return out;
    }

    // addition: Hits and the running-precision sum (Experiment.cs:121-128) of the same K walks against one test set each,
    // evaluated on the device without writing a ranked list (rwr_recommend_restart_eval_batch).  topN > 0 evaluates the first
    // topN entries of every list, topN <= 0 the whole list
    struct RestartEval {
        std::vector<int64_t> nHits;
        std::vector<double> sumPrecision;
        std::vector<int64_t> listLen;
    };
    RestartEval recommendRestartEvalBatch(const std::vector<std::vector<int>> &nodes, const std::vector<std::vector<double>> &weights,
                                          const std::vector<int> &start, double dampingFactor, int nIteration,
                                          const std::vector<std::vector<int64_t>> &testSets, int topN = 0,
                                          const std::vector<std::vector<int>> *exclude = nullptr)
    {
        const int32_t K = (int32_t)nodes.size();
        if (weights.size() != nodes.size() || testSets.size() != nodes.size() || (!start.empty() && start.size() != nodes.size()) ||
            (exclude && exclude->size() != nodes.size()))
            throw std::invalid_argument("recommendRestartEvalBatch: nodes, weights, start, testSets and exclude must hold one entry per vector");
        std::vector<int64_t> ptr((size_t)K + 1, 0), eptr((size_t)K + 1, 0), tptr((size_t)K + 1, 0), tids;
        std::vector<int32_t> idx, eidx;
        std::vector<double> val;
        for (int32_t k = 0; k < K; ++k) {
            if (nodes[k].size() != weights[k].size())
                throw std::invalid_argument("recommendRestartEvalBatch: a restart vector's nodes and weights differ in length");
            idx.insert(idx.end(), nodes[k].begin(), nodes[k].end());
            val.insert(val.end(), weights[k].begin(), weights[k].end());
            ptr[(size_t)k + 1] = (int64_t)idx.size();
            if (exclude) eidx.insert(eidx.end(), (*exclude)[k].begin(), (*exclude)[k].end());
            eptr[(size_t)k + 1] = (int64_t)eidx.size();
            tids.insert(tids.end(), testSets[k].begin(), testSets[k].end());
            tptr[(size_t)k + 1] = (int64_t)tids.size();
        }
        std::vector<int32_t> st(start.begin(), start.end());
        RestartEval out{std::vector<int64_t>((size_t)K), std::vector<double>((size_t)K), std::vector<int64_t>((size_t)K)};
        check(rwr_recommend_restart_eval_batch(graph_.handle(), K, ptr.data(), idx.data(), val.data(), st.empty() ? nullptr : st.data(),
                                               exclude ? eptr.data() : nullptr, eidx.data(), dampingFactor, nIteration, topN,
                                               tptr.data(), tids.data(), out.nHits.data(), out.sumPrecision.data(), out.listLen.data()));
        return out;
    }

private:
    // the arrays the audience set entries take (every array holds at least one element, so that its pointer is valid)
    struct AudienceSets {
        int32_t K = 0, nPool = -1;
        uint32_t mask = 0;
        std::vector<int64_t> sp, dp;
        std::vector<int32_t> si, pool, di;
        std::vector<double> sw;
    };
    static AudienceSets packAudienceSets_(const std::vector<std::vector<int>> &sets, const std::vector<std::vector<double>> *weights,
                                          const std::vector<EdgeType> &exclEdgeTypes, const std::vector<int> *pool,
                                          const std::vector<std::vector<int>> *deny)
    {
        AudienceSets a;
        a.K = (int32_t)sets.size();
        if (weights && weights->size() != sets.size()) throw std::invalid_argument("audience sets: one weight list per set");
        if (deny && deny->size() != sets.size()) throw std::invalid_argument("audience sets: one deny list per set");
        for (EdgeType t : exclEdgeTypes) a.mask |= 1u << (unsigned)t;
        a.sp.assign(1, 0);
        a.dp.assign(1, 0);
        for (size_t k = 0; k < sets.size(); ++k) {
            if (weights && (*weights)[k].size() != sets[k].size()) throw std::invalid_argument("audience sets: one weight per member");
            a.si.insert(a.si.end(), sets[k].begin(), sets[k].end());
            if (weights) a.sw.insert(a.sw.end(), (*weights)[k].begin(), (*weights)[k].end());
            a.sp.push_back((int64_t)a.si.size());
            if (deny) a.di.insert(a.di.end(), (*deny)[k].begin(), (*deny)[k].end());
            a.dp.push_back((int64_t)a.di.size());
        }
        if (pool) { a.nPool = (int32_t)pool->size(); a.pool.assign(pool->begin(), pool->end()); }
        a.si.push_back(0); a.sw.push_back(0.0); a.pool.push_back(0); a.di.push_back(0);
        return a;
    }

    Graph &graph_;
};

}  // namespace RWRBased
}  // namespace Recommenders
