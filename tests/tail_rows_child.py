"""Cases of tests/test_gpu_tail_rows.py, and its child process: batched Recommendation over graphs that are NOT bipartite
(items linking items, users linking users, dangling rows, UNDEFINED- and ETC-typed nodes and links), at several tile widths
and iteration counts, with and without ITEM seeds, before and after rwr_graph_update_links -- every result compared bit for
bit with the C restatement of the reference.  librwr reads RWR_TAIL_ROWS / RWR_SPMM once per process, so the test starts
this script with them set; it prints TAIL_ROWS_CHILD_OK <cases> <digest of every result>."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle.c_oracle import FlatGraph                   # noqa: E402
from tests import graphgen as gg                        # noqa: E402

T_VALUES = (1, 2, 3, 5, 10)
TILE_WIDTHS = (8, 16, 32, 64)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def mixed_graph(seed, n=1500, n_links=16000, uniform=False):
    """Node types USER / ITEM / ETC / UNDEFINED in random order; links of every type between nodes of every type (items
    link items, users link users, UNDEFINED links in between); about one row in twelve has no out-link at all."""
    rng = np.random.default_rng(seed)
    node_type = rng.choice([gg.NODE_USER, gg.NODE_ITEM, gg.NODE_ETC, gg.NODE_UNDEFINED], size=n,
                           p=[0.40, 0.45, 0.10, 0.05]).astype(np.uint8)
    node_id = rng.permutation(np.arange(500, 500 + 3 * n, 3, dtype=np.int64))
    silent = rng.random(n) < 0.08                       # dangling rows
    lists = [[] for _ in range(n)]
    seen = [set() for _ in range(n)]

    def add(a, b, ty):
        if silent[a] or (b, ty) in seen[a]:             # DataLoader.addLink de-duplicates on (target, type)
            return
        seen[a].add((b, ty))
        lists[a].append((b, ty, 1.0 if uniform else float(rng.choice([0.5, 1.0, 2.0, 3.25]))))

    users = np.flatnonzero(node_type == gg.NODE_USER)
    items = np.flatnonzero(node_type == gg.NODE_ITEM)
    for _ in range(n_links // 2):                       # LIKE both ways, skewed towards the first users / items
        u = users[int(rng.random() * rng.random() * len(users))]
        v = items[int(rng.random() * rng.random() * len(items))]
        add(u, v, gg.EDGE_LIKE)
        add(v, u, gg.EDGE_LIKE)
    for _ in range(n_links // 4):                       # anything to anything, every link type
        a, b = (int(x) for x in rng.integers(0, n, 2))
        if a != b:
            add(a, b, int(rng.integers(0, 8)))
    for _ in range(n_links // 8):                       # items linking items, users linking users
        pool = items if rng.random() < 0.5 else users
        a, b = (int(x) for x in rng.choice(pool, 2))
        if a != b:
            add(a, b, gg.EDGE_ETC if pool is items else gg.EDGE_FRIENDSHIP)
    rowptr = np.zeros(n + 1, dtype=np.int64)
    dst, etype, w = [], [], []
    for i in range(n):
        for (t, y, wt) in lists[i]:
            dst.append(t); etype.append(y); w.append(wt)
        rowptr[i + 1] = len(dst)
    return dict(node_id=node_id, node_type=node_type, rowptr=rowptr, dst=np.array(dst, dtype=np.int32),
                etype=np.array(etype, dtype=np.uint8), w=np.array(w, dtype=np.float64))


def seed_sets(g, rng):
    """(name, seeds): no ITEM seed (the last step runs without a seed-row chain, the one before on the in-link sources of
    the ITEM rows), a single ITEM seed among users (one tile group keeps its last chain), many ITEM seeds."""
    nt = g["node_type"]
    non_items = np.flatnonzero(nt != gg.NODE_ITEM)
    items = np.flatnonzero(nt == gg.NODE_ITEM)
    a = rng.choice(non_items, 40, replace=False).astype(np.int32)
    b = a.copy()
    b[17] = items[3]
    c = np.concatenate([rng.choice(items, 30, replace=False), rng.choice(non_items, 10, replace=False)]).astype(np.int32)
    return [("no-item-seed", a), ("one-item-seed", b), ("item-seeds", c)]


def retarget_item_links(g, rng):
    """New link types that change which rows link into ITEM rows: every link into an ITEM row of 25 sources becomes
    UNDEFINED, 25 UNDEFINED links into ITEM rows become LIKE, and 40 raw weights change."""
    nt, rp, dst, et = g["node_type"], g["rowptr"], g["dst"], g["etype"].copy()
    w = g["w"].copy()
    into_item = nt[dst] == gg.NODE_ITEM
    src = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    cut = rng.choice(np.unique(src[into_item & (et != gg.EDGE_UNDEFINED)]), 25, replace=False)
    idx_cut = np.flatnonzero(into_item & np.isin(src, cut))
    et[idx_cut] = gg.EDGE_UNDEFINED
    und = np.flatnonzero(into_item & (g["etype"] == gg.EDGE_UNDEFINED) & ~np.isin(src, cut))
    idx_add = rng.choice(und, min(25, len(und)), replace=False)
    et[idx_add] = gg.EDGE_LIKE
    idx_w = rng.choice(np.setdiff1d(np.arange(len(dst)), np.concatenate([idx_cut, idx_add])), 40, replace=False)
    if len(np.unique(w)) > 1:                           # (a uniform graph keeps its equal weights)
        w[idx_w] = rng.choice([0.25, 4.0], size=len(idx_w))
    idx = np.concatenate([idx_cut, idx_add, idx_w])
    g2 = dict(g, etype=et, w=w)
    return g2, idx


def run_all(amd, log=None):
    """Runs every case against the oracle; returns (cases, sha256 of all results)."""
    h = hashlib.sha256()
    cases = 0
    for gname, gseed, uniform in (("weighted", 31, False), ("uniform", 32, True)):
        g = mixed_graph(gseed, uniform=uniform)
        rng = np.random.default_rng(gseed)
        sets = seed_sets(g, rng)
        g2, idx = retarget_item_links(g, rng)
        for G_w in TILE_WIDTHS:
            for tile_group in (0, 1):                   # one tile group for the batch / one per tile
                G = amd.Graph.from_flat(**g, tile_seeds=G_w, tile_group=tile_group)
                G.buildGraph()
                assert G.stats()["uniform_path"] == (1 if uniform else 0), (gname, G.stats())
                for phase, gg_ in (("built", g), ("updated", g2)):
                    if phase == "updated":
                        G.updateLinks(idx, etype=g2["etype"][idx], w=g2["w"][idx])
                    F = FlatGraph(**gg_)
                    rec = amd.Recommender(G)
                    for sname, seeds in sets:
                        for T in T_VALUES:
                            if tile_group == 1 and T not in (1, 2, 5):
                                continue
                            bi, bs, bc = rec.RecommendationBatch(seeds, 0.15, T, 20)
                            oi, os_, oc = F.recommend_batch(seeds, 0.15, T, 20)
                            what = (gname, phase, G_w, tile_group, sname, T)
                            assert (bc == oc).all(), (what, "counts differ")
                            assert (bi == oi).all(), (what, "ids differ")
                            assert (bits(bs) == bits(os_)).all(), (what, "scores not bitwise equal")
                            for a in (bi, bs, bc):
                                h.update(np.ascontiguousarray(a).tobytes())
                            cases += 1
                G.close()
    return cases, h.hexdigest()


def main():
    import recommendersystems_amd as amd
    cases, digest = run_all(amd)
    print("TAIL_ROWS_CHILD_OK", cases, digest)


if __name__ == "__main__":
    main()
