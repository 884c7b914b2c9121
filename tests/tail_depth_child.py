"""Cases of tests/test_gpu_tail_depth.py, and its child process: a batch's last steps walk row lists up to four levels deep,
and a step's seed-row chain runs only where the seed's row can still reach a row the ranking reads.  Every
result is compared bit for bit with the C restatement of the reference, for T = 1 .. 10 and tile widths 8-64: on bipartite
like-graphs with user seeds (four levels taken), with seeds that link into an item they do not like through a non-LIKE link
(the chain of step T - 1 runs), that LIKE an item and link it once more under another type (it may be skipped), whose only
item links are UNDEFINED, that are ITEM rows or dangling; on the non-bipartite mixed graphs; and after rwr_graph_update_links
turns a LIKE link into ETC and back.  librwr reads RWR_TAIL_ROWS / RWR_TAIL_DEPTH once per process, so the test starts this
script with them set; it prints TAIL_DEPTH_CHILD_OK <cases> <digest of every result>."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle.c_oracle import FlatGraph                   # noqa: E402
from tests import graphgen as gg                        # noqa: E402
from tests.tail_rows_child import bits, mixed_graph     # noqa: E402

T_VALUES = tuple(range(1, 11))
TILE_WIDTHS = (8, 16, 32, 64)
D = 0.15


def like_graph(seed, n_users=700, n_items=2300, n_likes=7000):
    """A bipartite like-graph (users LIKE items, items LIKE users back), sparse enough for the frontier-list steps, with a few
    users whose links are special: `purchase` also links an item it does not like (PURCHASE), `both` links an item it likes
    a second time (PURCHASE), `undefined` links items only through UNDEFINED links and a user through FRIENDSHIP, `dangling`
    has no link at all.  Returns (graph, {role: user row})."""
    rng = np.random.default_rng(seed)
    n = n_users + n_items
    node_type = np.concatenate([np.full(n_users, gg.NODE_USER), np.full(n_items, gg.NODE_ITEM)]).astype(np.uint8)
    node_id = rng.permutation(np.arange(100, 100 + 2 * n, 2, dtype=np.int64))
    roles = {"purchase": 3, "both": 5, "undefined": 8, "dangling": 11}
    lists = [dict() for _ in range(n)]   # target -> [types], insertion-ordered
    for _ in range(n_likes):
        u = int(rng.random() * rng.random() * n_users)
        v = n_users + int(rng.random() * n_items)
        if u in (roles["undefined"], roles["dangling"]) or gg.EDGE_LIKE in lists[u].get(v, []):
            continue
        lists[u].setdefault(v, []).append(gg.EDGE_LIKE)
        lists[v].setdefault(u, []).append(gg.EDGE_LIKE)
    p = roles["purchase"]
    while True:
        v = n_users + int(rng.integers(0, n_items))
        if v not in lists[p]:
            lists[p][v] = [gg.EDGE_PURCHASE]
            break
    b = roles["both"]
    lists[b][next(iter(lists[b]))].append(gg.EDGE_PURCHASE)
    u = roles["undefined"]
    for v in rng.choice(np.arange(n_users, n), 5, replace=False):
        lists[u][int(v)] = [gg.EDGE_UNDEFINED]
    lists[u][1] = [gg.EDGE_FRIENDSHIP]
    rowptr = np.zeros(n + 1, dtype=np.int64)
    dst, etype = [], []
    for i in range(n):
        for t, tys in lists[i].items():
            for ty in tys:
                dst.append(t)
                etype.append(ty)
        rowptr[i + 1] = len(dst)
    g = dict(node_id=node_id, node_type=node_type, rowptr=rowptr, dst=np.array(dst, dtype=np.int32),
             etype=np.array(etype, dtype=np.uint8), w=np.ones(len(dst), dtype=np.float64))
    return g, roles


def like_seed_sets(g, roles, rng):
    nt, rp = g["node_type"], g["rowptr"]
    users = np.flatnonzero((nt == gg.NODE_USER) & (np.diff(rp) > 0))
    users = np.setdiff1d(users, list(roles.values()))
    items = np.flatnonzero((nt == gg.NODE_ITEM) & (np.diff(rp) > 0))
    base = rng.choice(users, 40, replace=False).astype(np.int32)

    def with_(row, at=17):
        s = base.copy()
        s[at] = row
        return s
    return [("users", base), ("purchase", with_(roles["purchase"])), ("both", with_(roles["both"])),
            ("undefined", with_(roles["undefined"])), ("item", with_(items[4])), ("dangling", with_(roles["dangling"]))]


def check(rec, F, seeds, T, what, h, top_n=20):
    bi, bs, bc = rec.RecommendationBatch(seeds, D, T, top_n)
    oi, os_, oc = F.recommend_batch(seeds, D, T, top_n)
    assert (bc == oc).all(), (what, "counts differ")
    assert (bi == oi).all(), (what, "ids differ")
    assert (bits(bs) == bits(os_)).all(), (what, "scores not bitwise equal")
    for a in (bi, bs, bc):
        h.update(np.ascontiguousarray(a).tobytes())


def expected_launches(seed_set):
    """(dense SpMM launches, seed-row chains) of one T = 10 tile group on the like-graph, under this process's settings:
    steps 0-3 probe the frontier bitmaps, steps T - k walk row lists while k <= the last restricted level."""
    if os.environ.get("RWR_TAIL_ROWS") == "0":
        return 6, 10
    depth = int(os.environ.get("RWR_TAIL_DEPTH", "4"))
    # the first level whose chain a seed of the set needs (bit k of the tail flags), or depth - 1
    first = {"users": 3, "purchase": 1, "both": 3, "undefined": 2, "item": 0, "dangling": 3}[seed_set]
    last = min(first, depth - 1)
    restricted = last + 1
    chains = 10 - restricted + (1 if first <= depth - 1 else 0)
    return 10 - 4 - restricted, chains


def launches(G):
    st = G.stats()
    return st["spmm_dense_launches"], st["chain_launches"], st["spmm_launches"]


def run_all(amd):
    """Runs every case against the oracle; returns (cases, sha256 of all results)."""
    h = hashlib.sha256()
    cases = 0
    fl = 0
    # bipartite like-graphs
    for gname, gseed in (("like", 51), ("like2", 52)):
        g, roles = like_graph(gseed)
        F = FlatGraph(**g)
        rng = np.random.default_rng(gseed)
        sets = like_seed_sets(g, roles, rng)
        for G_w in TILE_WIDTHS:
            for tile_group in (0, 1):                   # one tile group for the batch / one per tile
                G = amd.Graph.from_flat(**g, tile_seeds=G_w, tile_group=tile_group)
                G.buildGraph()
                rec = amd.Recommender(G)
                for sname, seeds in sets:
                    for T in T_VALUES:
                        if tile_group == 1 and T not in (1, 3, 4, 5, 10):
                            continue
                        before = launches(G)
                        check(rec, F, seeds, T, (gname, G_w, tile_group, sname, T), h)
                        after = launches(G)
                        if T == 10 and tile_group == 0 and sname != "dangling":   # (one tile group for all 40 seeds)
                            got = tuple(x - y for x, y in zip(after, before))
                            assert got == expected_launches(sname) + (10,), (gname, G_w, sname, got)
                        cases += 1
                # dangling seeds iterated with the others (a list longer than the selection's shortcut)
                if tile_group == 0 and G_w == 32:
                    for T in (2, 4, 6):
                        check(rec, F, sets[5][1], T, (gname, G_w, "dangling-iterated", T), h, top_n=1100)
                        cases += 1
                fl += G.stats()["frontier_list_launches"]
                G.close()
        # rwr_graph_update_links: a user's LIKE of an item becomes ETC -- an explicit link into an item it no longer likes, so
        # its chain of step T - 1 must run -- then LIKE again
        G = amd.Graph.from_flat(**g, tile_seeds=64)
        G.buildGraph()
        rec = amd.Recommender(G)
        seeds = sets[0][1]
        idx = np.array([g["rowptr"][seeds[3]]], dtype=np.int64)
        assert g["etype"][idx[0]] == gg.EDGE_LIKE
        for phase, ty in (("etc", gg.EDGE_ETC), ("like", gg.EDGE_LIKE)):
            G.updateLinks(idx, etype=np.array([ty], dtype=np.uint8), w=g["w"][idx])
            g2 = dict(g, etype=g["etype"].copy())
            g2["etype"][idx] = ty
            F2 = FlatGraph(**g2)
            for T in T_VALUES:
                before = launches(G)
                check(rec, F2, seeds, T, (gname, "updated", phase, T), h)
                after = launches(G)
                if T == 10:
                    got = tuple(x - y for x, y in zip(after, before))
                    assert got == expected_launches("purchase" if phase == "etc" else "users") + (10,), (gname, phase, got)
                cases += 1
        G.close()
    # non-bipartite graphs: items link items, users link users, every link type, dangling rows
    for gname, gseed, uniform in (("weighted", 61, False), ("uniform", 62, True)):
        g = mixed_graph(gseed, uniform=uniform)
        F = FlatGraph(**g)
        rng = np.random.default_rng(gseed)
        nt = g["node_type"]
        non_items = np.flatnonzero(nt != gg.NODE_ITEM)
        items = np.flatnonzero(nt == gg.NODE_ITEM)
        a = rng.choice(non_items, 40, replace=False).astype(np.int32)
        c = np.concatenate([rng.choice(items, 5, replace=False), rng.choice(non_items, 35, replace=False)]).astype(np.int32)
        for G_w in TILE_WIDTHS:
            G = amd.Graph.from_flat(**g, tile_seeds=G_w)
            G.buildGraph()
            rec = amd.Recommender(G)
            for sname, seeds in (("no-item-seed", a), ("item-seeds", c)):
                for T in T_VALUES:
                    check(rec, F, seeds, T, (gname, G_w, sname, T), h)
                    cases += 1
            G.close()
    if os.environ.get("RWR_TAIL_ROWS") != "0":
        assert fl > 0, "no frontier-list launch ran"
    return cases, h.hexdigest()


def main():
    import recommendersystems_amd as amd
    cases, digest = run_all(amd)
    print("TAIL_DEPTH_CHILD_OK", cases, digest)


if __name__ == "__main__":
    main()
