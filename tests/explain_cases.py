"""Graphs, cases and the expectation model of the explained entry's tests (rwr_recommend_explained_batch).  Nothing here
touches the library: the expectation is built from the rank rows of oracle/rwr_oracle.py's Model at T and at T - 1 (through
tests/test_gpu_typed.py's oracle_row), the normalised weights of the oracle's Graph.graph, the addends formed in float64 with two
separately rounded products, and the lists of tests/test_gpu_capped.py's filtered_rows / greedy in the (-score, -id, row) order.
tests/test_explain_cases.py proves on the CPU that the model is the reference's arithmetic and that every case bites;
tests/test_gpu_explained.py compares the library with it."""
import numpy as np

from oracle import rwr_oracle as po
from tests import graphgen as gg
from tests import test_gpu_typed as tt
from tests.test_gpu_capped import filtered_rows, greedy
from tests.test_gpu_typed import _flat, _mixed, oracle_row

D = tt.D
WHY_MAX = 8                # RWR_WHY_MAX, include/rwr.h
WHY_BLOCK = 256            # explain.hip: the lanes that share one entry
C1 = 1 - po.widen_float(D)  # Model.cs:84 with d = (double)(float)D

# in-degrees of the crafted graph's items, by users: 0, 1, n_why - 1 .. n_why + 1 for n_why in {1, 2, 8}, the wave's edge, the
# workgroup's edge, and one hub above twice the lanes that share an entry
DEGREES = [0, 1, 2, 3, 7, 8, 9, 63, 64, 65, 4, 5, 6, 10, 16, 33, 100, 255, 256, 257, 513, 700]
HUB = 700
N_USERS = 800


def crafted(uniform):
    """N_USERS users and len(DEGREES) + 1 items: item i is liked by exactly DEGREES[i] users; the last item by 12 users, one of
    them through two parallel links.  Every like has a MENTION link back (item -> user), so users have in-lists too.  Returns
    (graph, rows of the items)."""
    rng = np.random.default_rng(5 if uniform else 4)
    n_items = len(DEGREES) + 1
    items = list(range(N_USERS, N_USERS + n_items))
    lists = [[] for _ in range(N_USERS + n_items)]
    weight = (lambda: 1.0) if uniform else (lambda: float(rng.integers(1, 9)) / 4.0)
    for i, deg in enumerate(DEGREES + [12]):
        users = np.sort(rng.choice(N_USERS, deg, replace=False))
        for u in users:
            lists[int(u)].append((items[i], gg.EDGE_LIKE, weight()))
            lists[items[i]].append((int(u), gg.EDGE_MENTION, weight()))
        if i == len(DEGREES):
            lists[int(users[3])].append((items[i], gg.EDGE_LIKE, weight()))   # the parallel link: its own in-entry
    ids = np.concatenate([np.arange(N_USERS) + 1000, 5000 - np.arange(n_items)])
    types = np.array([gg.NODE_USER] * N_USERS + [gg.NODE_ITEM] * n_items)
    return _flat(ids, types, lists), items


def with_twins(g):
    """two more ITEM nodes with one and the same id and no links: both score 0 for every seed"""
    lists = tt._lists(g) + [[], []]
    return _flat(np.concatenate([g["node_id"], [77777, 77777]]), np.concatenate([g["node_type"], [gg.NODE_ITEM, gg.NODE_ITEM]]), lists)


_graphs = {}


def graph(name):
    if name not in _graphs:
        if name in ("hub_w", "hub_u"):
            _graphs[name] = crafted(name == "hub_u")[0]
        elif name in ("mixed", "unit"):
            _graphs[name] = _mixed(11 if name == "mixed" else 12, uniform=name == "unit")[0]
        elif name == "twins":
            _graphs[name] = with_twins(graph("mixed"))
    return _graphs[name]


# ---- the expectation ---------------------------------------------------------------------------------------------------------------

_in_lists = {}


def in_lists(g):
    """per node the in-entries (source, normalised weight) in the addend order of Model.deliverRanks: source ascending, then
    list position ascending; from the oracle's Graph.graph, which holds the explicit links only"""
    if id(g) not in _in_lists:
        oracle_row(g, 0, 0)
        G = tt._oracle_graphs[id(g)][0]
        inl = [[] for _ in range(len(g["node_id"]))]
        for u in range(len(inl)):
            for link in G.graph[u] or ():
                inl[link.targetNode].append((u, link.weight))
        _in_lists[id(g)] = inl
    return _in_lists[id(g)]


def addends(g, seed, T, v):
    """[(source, a_e)] of v's in-entries over the previous ranks; T <= 0: no step ran"""
    if T <= 0:
        return []
    y = oracle_row(g, int(seed), T - 1)
    out = []
    for u, w in in_lists(g)[v]:
        rw = C1 * float(y[u])                                      # Model.cs:84, rounded
        out.append((u, rw * w))                                    # Model.cs:87's product, rounded
    return out


def reasons(adds):
    """the in-list positions of the positive addends, best first: value descending, then position ascending"""
    return sorted((e for e, (_, a) in enumerate(adds) if a > 0), key=lambda e: (-adds[e][1], e))


def list_rows(g, case):
    """per batch position the rows of the list the capped entry defines, in the (-score, -id, row) order, cut to top_n"""
    out = []
    for k, s in enumerate(case["seeds"]):
        row = oracle_row(g, int(s), case["T"])
        deny = () if case.get("deny") is None else case["deny"][k]
        F = filtered_rows(g, row, int(s), case.get("cand"), set(case.get("edges", ())), case.get("self", False), case.get("pool"), deny)
        out.append(greedy(F, case.get("lab"), case.get("m", 1))[:case["top_n"]])
    return out


def expected(g, case):
    """(ids, scores, counts, nodes, why_src, why_term, why_total) as the header defines them"""
    K, top_n, r, T = len(case["seeds"]), case["top_n"], case["n_why"], case["T"]
    ids, sc, cnt = np.zeros((K, top_n), dtype=np.int64), np.zeros((K, top_n)), np.zeros(K, dtype=np.int32)
    nodes = np.full((K, top_n), -1, dtype=np.int32)
    src, term = np.full((K, top_n, r), -1, dtype=np.int32), np.zeros((K, top_n, r))
    total = np.zeros((K, top_n), dtype=np.int64)
    for k, L in enumerate(list_rows(g, case)):
        s = int(case["seeds"][k])
        row = oracle_row(g, s, T)
        cnt[k] = len(L)
        for j, v in enumerate(L):
            ids[k, j], sc[k, j], nodes[k, j] = int(g["node_id"][v]), float(row[v]), v
            adds = addends(g, s, T, v)
            best = reasons(adds)
            total[k, j] = len(best)
            for i, e in enumerate(best[:r]):
                src[k, j, i], term[k, j, i] = adds[e]
    return ids, sc, cnt, nodes, src, term, total


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
# graph, seeds, T, top_n, n_why; cand (None: any type), edges (the mask), self, pool, deny, lab / m (the cap), opts (the handle's),
# env; bites: the properties tests/test_explain_cases.py proves from the reference alone

USER, ITEM = gg.NODE_USER, gg.NODE_ITEM


def _case(name, graph, seeds, T, top_n, n_why, bites=(), **kw):
    return dict(name=name, graph=graph, seeds=list(seeds), T=T, top_n=top_n, n_why=n_why, bites=tuple(bites), **kw)


def _cases():
    out = []
    # every in-degree at every n_why: all items listed (top_n beyond the list: unused cells), the hub, in-degree 0
    for r in (1, 2, 8):
        out.append(_case("hub_w-r%d" % r, "hub_w", [0, 5, 5, 799], 3, 40, r, ("hub", "trunc", "short", "zero"), cand=ITEM))
    out.append(_case("hub_w-rows-only", "hub_w", [3], 3, 40, 0, ("short",), cand=ITEM))
    # the uniform graph: equal addends straddle position n_why, in-list position decides
    for T in (2, 3):
        out.append(_case("hub_u-T%d" % T, "hub_u", [1, 2, 640], T, 30, 2, ("short",) + (("tie", "trunc") if T == 3 else ()), cand=ITEM))
    out.append(_case("hub_u-T10-r8", "hub_u", [7], 10, 5, 8, ("tie", "trunc"), cand=ITEM, opts=dict(tile_seeds=1)))
    # T: no step, the seed as the only reason, a Y with stale rows would show at 2 and 3
    for name in ("mixed", "unit"):
        for T in (0, 1, 2, 3, 10):
            out.append(_case("%s-T%d" % (name, T), name, [2, 326, 2, 9, 327], T, 12, 3, ("zero",) if T == 0 else (), cand=None,
                             opts=dict(tile_seeds=8, tile_group=1)))
    # tile widths and several tile groups, duplicate and dangling seeds
    out.append(_case("mixed-K65-g8", "mixed", [(7 * k) % 120 for k in range(63)] + [326, 327], 3, 10, 3, cand=ITEM, edges=(gg.EDGE_LIKE,),
                     opts=dict(tile_seeds=8, tile_group=1)))
    out.append(_case("unit-K3-g1", "unit", [4, 4, 326], 3, 10, 3, cand=ITEM, opts=dict(tile_seeds=1, tile_group=1)))
    out.append(_case("mixed-K65-g64", "mixed", [(11 * k) % 120 for k in range(65)], 2, 6, 2, cand=USER, self=True, edges=(gg.EDGE_FOLLOW,),
                     opts=dict(tile_seeds=64, tile_group=1)))
    # top_n: one entry; the select's largest list on a graph of 330 nodes
    out.append(_case("mixed-top1", "mixed", [0, 1, 2], 3, 1, 8, cand=ITEM))
    out.append(_case("mixed-top1024", "mixed", [6], 3, 1024, 1, ("short", "zero"), cand=None))
    # the seed as its own entry: link addends only
    out.append(_case("mixed-self", "mixed", [2, 30], 3, 5, 8, ("self",), cand=USER, self=False))
    # a pool, a deny list and a cap together (a small chunk: the cap's split form)
    g = graph("mixed")
    items = np.flatnonzero(g["node_type"] == ITEM)
    lab = np.full(len(g["node_id"]), -1, dtype=np.int32)
    lab[items] = np.arange(items.size) % 4
    out.append(_case("mixed-composed", "mixed", [1, 8, 15], 3, 20, 3, ("capped",), cand=ITEM, edges=(gg.EDGE_LIKE,), pool=items[::2].tolist(),
                     deny=[items[:6:2].tolist(), [], items[10:40:2].tolist()], lab=lab, m=2, env=dict(RWR_CAP_CHUNK="8")))
    # equal (score, id) pairs: the smaller row first
    out.append(_case("twins", "twins", [3, 9], 2, 330, 1, ("twins", "zero"), cand=ITEM))
    return out


CASES = _cases()
