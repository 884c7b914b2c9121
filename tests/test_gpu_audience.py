"""rwr_recommend_audience_batch on the GPU against the NumPy forward reference of tests/audience_cases.py -- the
literal Model.cs loop from EVERY node as a seed -- with the list comparison that is safe under the derived tolerance: scores
within tol_rel of the forward values (+0.0 on +0.0), the list sorted by its own keys, no candidate left out that beats the
last entry, excluded nodes absent, the counts exact.  Varied: the batch shape (one column, a full tile, a tile plus one, a
padded third tile; repeated targets; alone against inside a batch, bitwise), the walk (T and d), crafted out-degrees around the
loop-free path and the long-row split, graphs without and with mostly dangling nodes, weighted and value-free graphs, the
selection (mask, exclude_self, cand_type, top_n), the handle after rwr_graph_remove_nodes and rwr_graph_append_nodes, and the
duality with rwr_recommend_typed_positions_batch from every user."""
import numpy as np
import pytest

from tests import audience_cases as ac
from tests import graphgen as gg

pytestmark = pytest.mark.gpu

LIKE, UNDEF = 1 << gg.EDGE_LIKE, 1 << gg.EDGE_UNDEFINED
SPLIT = 512                                                      # audience_plan.h: AUD_SPLIT
_REF = {}


def f32(d):
    return float(np.float32(d))                                  # the entry takes a float and widens it


def _api():
    from recommendersystems_amd.rwr_based import Graph, Recommender
    return Graph, Recommender


def opened(g):
    Graph, Recommender = _api()
    G = Graph.from_flat(**g)
    G.buildGraph()
    return G, Recommender(G)


def graph(name):
    if name not in _REF:
        if name == "mix":
            g = gg.random_graph(21, n_users=120, n_items=260, n_likes=1500, n_etc=6, n_friend=60, n_mention=50, n_author=30)
        elif name == "uni":
            g = gg.random_graph(22, n_users=100, n_items=240, n_likes=1300, uniform=True)
        elif name == "deg":
            g = ac.degree_graph([0, 1, 4, 5, 63, 64, 65, SPLIT - 1, SPLIT, SPLIT + 1, 2 * SPLIT + 40, 3, 2, 0], 23,
                                n_items=2 * SPLIT + 120, back_every=2)
        elif name == "deg_uni":
            g = ac.degree_graph([0, 1, 4, 5, 63, 64, 65, SPLIT - 1, SPLIT, SPLIT + 1, 3], 24, n_items=SPLIT + 60, weighted=False,
                                p_undefined=0.0)
        elif name == "nodang":
            g = ac.drop_dangling(gg.random_graph(25, n_users=90, n_items=200, n_likes=1000, n_friend=40, n_mention=30))
        else:
            raise KeyError(name)
        _REF[name] = (g,) + ac.normalise(g)
    return _REF[name]


def reference(name, T, d):
    """F[s, v] = x_T^(s)[v] for every pair, computed once per (graph, T, d)"""
    key = (name, T, d)
    if key not in _REF:
        g, wn, nd = graph(name)
        _REF[key] = ac.forward(g, wn, nd, np.arange(len(nd)), T, d)
    return _REF[key]


def audience(rec, g, F, targets, T, d, cand=None, mask=0, self_=False, top_n=100):
    ids, sc, nodes, cnt = rec.AudienceBatch(np.asarray(targets, dtype=np.int32), d, T, cand, mask, self_, top_n)
    tol = ac.tol_rel(g, T, d)
    worst = 0.0
    for k, v in enumerate(targets):
        worst = max(worst, ac.check_list(g, F[:, v], ids[k], sc[k], nodes[k], int(cnt[k]), target=int(v), cand_type=cand, mask=mask,
                                         exclude_self=self_, top_n=top_n, tol=tol))
    print("largest relative error %.3g (tol %.3g)" % (worst, tol))
    return ids, sc.view(np.uint64), nodes, cnt


def special_targets(g, nd):
    """an item, a user, a dangling node, a node without in-links, the last node"""
    n = len(nd)
    indeg = np.bincount(g["dst"], minlength=n)
    t = g["node_type"]
    out = [int(np.nonzero((t == gg.NODE_ITEM) & (indeg > 3))[0][0]), int(np.nonzero((t == gg.NODE_USER) & (indeg > 0))[0][0])]
    if (~nd).any():
        out.append(int(np.nonzero(~nd)[0][-1]))
    if (indeg == 0).any():
        out.append(int(np.nonzero(indeg == 0)[0][0]))
    return out + [n - 1]


@pytest.mark.parametrize("K", [1, 16, 17, 33])
def test_batch_shapes(K):
    g, wn, nd = graph("mix")
    T, d = 10, f32(0.15)
    F = reference("mix", T, d)
    G, rec = opened(g)
    items = np.nonzero(g["node_type"] == gg.NODE_ITEM)[0]
    targets = [int(x) for x in items[np.arange(K) * 5 % len(items)]]
    if K > 1:
        targets[-1] = targets[0]                                 # a target that repeats owns two columns
    ids, sc, nodes, cnt = audience(rec, g, F, targets, T, d, gg.NODE_USER, LIKE, False, 100)
    if K > 1:
        assert (ids[-1] == ids[0]).all() and (sc[-1] == sc[0]).all() and (nodes[-1] == nodes[0]).all() and cnt[-1] == cnt[0]
    for k in sorted({0, K // 2, K - 1}):                         # alone and inside the batch: the same bits
        i1, s1, n1, c1 = audience(rec, g, F, [targets[k]], T, d, gg.NODE_USER, LIKE, False, 100)
        assert (i1[0] == ids[k]).all() and (s1[0] == sc[k]).all() and (n1[0] == nodes[k]).all() and c1[0] == cnt[k]
    again = audience(rec, g, F, targets, T, d, gg.NODE_USER, LIKE, False, 100)
    for a, b in zip(again, (ids, sc, nodes, cnt)):               # two consecutive calls
        assert (a == b).all()
    G.close()


@pytest.mark.parametrize("T", [0, 1, 2, 10])
@pytest.mark.parametrize("d", [0.15, 0.5, 1.0])
def test_walks(T, d):
    g, wn, nd = graph("mix")
    d = f32(d)
    F = reference("mix", T, d)
    G, rec = opened(g)
    audience(rec, g, F, special_targets(g, nd), T, d, None, 0, False, 1024)
    audience(rec, g, F, special_targets(g, nd)[:2], T, d, gg.NODE_USER, LIKE | UNDEF, True, 50)
    G.close()


@pytest.mark.parametrize("name", ["deg", "deg_uni", "uni", "nodang"])
def test_crafted_graphs(name):
    """out-degrees 0, 1, 4, 5, 63, 64, 65, the long-row split's edges and three pieces; half of the nodes dangling; UNDEFINED links
    inside lists; the value-free path; no dangling node at all (the constant-rho path)"""
    g, wn, nd = graph(name)
    n = len(nd)
    if name.startswith("deg"):
        assert int(np.diff(g["rowptr"]).max()) > SPLIT and (~nd).sum() * 2 >= n - 40
    if name == "nodang":
        assert nd.all()
    G, rec = opened(g)
    st = G.stats()
    assert bool(st["uniform_path"]) == (name in ("deg_uni", "uni"))
    for T, d in ((1, f32(0.5)), (3, f32(0.15))):
        F = reference(name, T, d)
        targets = special_targets(g, nd)
        # the items the longest rows link to, so that the long rows' sums are non-zero columns
        long_row = int(np.argmax(np.diff(g["rowptr"])))
        p0, p1 = int(g["rowptr"][long_row]), int(g["rowptr"][long_row + 1])
        targets += [int(g["dst"][p0]), int(g["dst"][p1 - 1]), int(g["dst"][(p0 + p1) // 2])]
        audience(rec, g, F, targets, T, d, None, 0, False, 1024)
        audience(rec, g, F, targets, T, d, gg.NODE_USER, LIKE, True, 7)
    G.close()


def test_selection():
    g, wn, nd = graph("mix")
    T, d = 3, f32(0.15)
    F = reference("mix", T, d)
    G, rec = opened(g)
    targets = special_targets(g, nd)
    n_users = int((g["node_type"] == gg.NODE_USER).sum())
    for mask in (0, LIKE, LIKE | UNDEF):
        for self_ in (False, True):
            for cand in (gg.NODE_USER, gg.NODE_ITEM, None):
                audience(rec, g, F, targets, T, d, cand, mask, self_, 100)
    for top_n in (1, 100, 1024):
        audience(rec, g, F, targets, T, d, None, LIKE, True, top_n)
    ids, sc, nodes, cnt = audience(rec, g, F, targets, T, d, gg.NODE_USER, 0, False, 1024)   # above the candidate count
    assert (cnt == n_users).all() and (nodes[:, n_users:] == -1).all()
    # d = 0 is legal: finite, >= 0, and the same twice
    a = rec.AudienceBatch(np.asarray(targets, dtype=np.int32), 0.0, 4, None, 0, False, 200)
    b = rec.AudienceBatch(np.asarray(targets, dtype=np.int32), 0.0, 4, None, 0, False, 200)
    assert np.isfinite(a[1]).all() and (a[1] >= 0).all()
    for x, y in zip(a, b):
        assert (x.view(np.uint8) == y.view(np.uint8)).all()
    G.close()


def test_duality_with_forward_positions():
    """s is in the whole audience list of v exactly when v is in the whole typed list of seed s, and the scores agree"""
    from recommendersystems_amd.rwr_based import EdgeType, NodeType
    g, wn, nd = graph("mix")
    T, d = 10, f32(0.15)
    G, rec = opened(g)
    users = np.nonzero(g["node_type"] == gg.NODE_USER)[0].astype(np.int32)
    indeg = np.bincount(g["dst"], minlength=len(nd))
    items = np.nonzero(g["node_type"] == gg.NODE_ITEM)[0]
    tol = ac.tol_rel(g, T, d)
    for v in (int(items[np.argmax(indeg[items])]), int(items[7])):
        ids, sc, nodes, cnt = rec.AudienceBatch([v], d, T, gg.NODE_USER, LIKE, True, 1024)
        c = int(cnt[0])
        assert c < 1024
        pos, fsc, _ = rec.RecommendationTypedPositionsBatch(users, d, T, [[int(g["node_id"][v])]] * len(users), NodeType.ITEM,
                                                            (EdgeType.LIKE,), True)
        forward_in = {int(u) for u, p in zip(users, pos) if p[0] >= 0}
        assert forward_in == {int(x) for x in nodes[0, :c]}
        fs = {int(u): float(s[0]) for u, s in zip(users, fsc)}
        for q in range(c):
            f, r = fs[int(nodes[0, q])], float(sc[0, q])
            assert (r == 0.0 and not np.signbit(r)) if f == 0.0 else abs(r - f) <= tol * f, (q, r, f)
    G.close()


def test_after_remove_and_append_nodes():
    """the same handle after rwr_graph_remove_nodes (indices renumbered, the candidate cache emptied) and after
    rwr_graph_append_nodes (the candidate lists rebuilt for the grown node set)"""
    from tests.test_gpu_graph_remove_nodes import grown, without
    from tests.test_gpu_graph_append import patched
    g, wn, nd = graph("mix")
    T, d = 3, f32(0.15)
    G, rec = opened(g)
    audience(rec, g, reference("mix", T, d), special_targets(g, nd), T, d, gg.NODE_USER, LIKE, True, 60)
    lost = [2, 57, 130, 131, 300]
    g2, _, _ = without(g, lost)
    G.removeNodes(np.asarray(lost, dtype=np.int32))
    wn2, nd2 = ac.normalise(g2)
    F2 = ac.forward(g2, wn2, nd2, np.arange(len(nd2)), T, d)
    audience(rec, g2, F2, special_targets(g2, nd2), T, d, gg.NODE_USER, LIKE, True, 60)
    audience(rec, g2, F2, special_targets(g2, nd2), T, d, None, LIKE | UNDEF, False, 1024)
    n2 = len(nd2)
    g3 = grown(g2, [777001, 777002], [gg.NODE_USER, gg.NODE_ITEM])
    g3, _ = patched(g3, [n2, n2, 5], [n2 + 1, 200, n2 + 1], [gg.EDGE_LIKE, gg.EDGE_LIKE, gg.EDGE_LIKE], [1.0, 2.0, 1.0])
    G.appendNodes([(777001, gg.NODE_USER), (777002, gg.NODE_ITEM)], [n2, n2, 5], [n2 + 1, 200, n2 + 1],
                  [gg.EDGE_LIKE, gg.EDGE_LIKE, gg.EDGE_LIKE], [1.0, 2.0, 1.0])
    wn3, nd3 = ac.normalise(g3)
    F3 = ac.forward(g3, wn3, nd3, np.arange(len(nd3)), T, d)
    audience(rec, g3, F3, special_targets(g3, nd3) + [n2 + 1, n2], T, d, gg.NODE_USER, LIKE, True, 60)
    audience(rec, g3, F3, [n2 + 1, 200], T, d, None, 0, False, 1024)
    G.close()
