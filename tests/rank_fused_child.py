"""Child process of tests/test_gpu_rank_fused.py: librwr reads RWR_RANK_FUSED, RWR_RANK_FUSED_HEAD, RWR_RANK_FUSED_CAP (and
RWR_VALUE_FREE) once per process, so every setting runs in a fresh interpreter.  Runs every case below through
RecommendationBatch, compares ids, scores and counts bitwise with the C restatement of the reference, and writes them -- with
the rank_fused_groups / rank_fused_fallbacks counters of each call -- to the .npz named on the command line, which the parent
compares with the file of the RWR_RANK_FUSED=0 child."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import recommendersystems_amd as amd                    # noqa: E402
from recommendersystems_amd import _lib                 # noqa: E402
from oracle.c_oracle import FlatGraph                   # noqa: E402
from tests import graphgen as gg                        # noqa: E402

USER, ITEM, LIKE = 1, 2, 1


def from_likes(n_users, n_items, likes, rng=None, weights=None):
    """Bipartite graph from (user, item) pairs: user rows hold their items, item rows their users (both LIKE, as the loader
    writes them); rng: shuffle every list; weights: per-link raw weights in place of 1.0."""
    likes = sorted(set(likes))
    n = n_users + n_items
    lists = [[] for _ in range(n)]
    for u, v in likes:
        lists[u].append(n_users + v)
        lists[n_users + v].append(u)
    if rng is not None:
        for l in lists:
            rng.shuffle(l)
    rowptr = np.zeros(n + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum([len(l) for l in lists])
    dst = np.array([t for l in lists for t in l], dtype=np.int32)
    node_type = np.array([USER] * n_users + [ITEM] * n_items, dtype=np.uint8)
    w = np.ones(len(dst)) if weights is None else weights(len(dst))
    # ids in no relation to the row order, so that "id descending" is not "row descending"
    ids = np.random.default_rng(99).permutation(n).astype(np.int64) * 7 + 3
    return dict(node_id=ids, node_type=node_type, rowptr=rowptr, dst=dst, etype=np.full(len(dst), LIKE, dtype=np.uint8),
                w=np.asarray(w, dtype=np.float64))


def tie_graph(n_items=1500, weights=None):
    """Three groups of 25 items with identical in-lists (30, 20 and 12 users: the three highest in-degrees of the graph, so
    that the groups open tail_rows[0] and a small head ends inside one), hence identical scores; random likes elsewhere;
    users 0..5 also like 30 cold items each that nobody else likes; user 199 likes nothing (dangling)."""
    rng = np.random.default_rng(17)
    U = 200
    likes = []
    for grp, fans in enumerate((range(10, 40), range(40, 60), range(60, 72))):
        likes += [(u, grp * 25 + j) for u in fans for j in range(25)]
    for u in range(U - 1):
        for v in rng.choice(np.arange(75, n_items - 180), size=int(rng.integers(2, 9)), replace=False):
            likes.append((u, int(v)))
    for u in range(6):
        likes += [(u, n_items - 180 + 30 * u + j) for j in range(30)]
    return from_likes(U, n_items, likes, rng, weights), U


def cases():
    """(name, graph, seeds, T, top_n, tile_seeds)"""
    g, U = tie_graph()
    live = np.array([0, 3, 5, 8, 12, 45, 66, 80, 100, 120, 150, 180, 190], dtype=np.int32)    # 13 seeds: padded slots at G = 8, 16
    for G in (8, 16, 32):
        for top_n in (5, 30, 60):
            yield f"tie-G{G}-top{top_n}", g, live, 10, top_n, G
    yield "tie-duplicates-dangling", g, np.array([3, 80, 3, 199, 45, 80, 3, 0, 12, 199], dtype=np.int32), 10, 5, 8
    yield "tie-item-seed", g, np.array([3, 80, U + 4, 45, 0, 12, 100, 120, 150], dtype=np.int32), 10, 5, 8
    for T in (1, 2, 3, 4):
        yield f"tie-T{T}", g, live, T, 5, 8
    yield "tie-top1025", g, live, 10, 1025, 8
    big, _ = tie_graph(n_items=6000)                       # more rows beyond a short head than a candidate buffer holds
    yield "big-top5", big, live, 10, 5, 16
    wg, _ = tie_graph(weights=lambda m: np.random.default_rng(5).choice([0.5, 1.0, 2.0, 3.25], size=m))
    yield "weighted-top5", wg, live, 10, 5, 8
    yield "weighted-top30", wg, live, 10, 30, 16
    yield "random-top20", gg.random_graph(21, n_users=400, n_items=1500, n_likes=9000, n_etc=10, n_friend=300, n_author=100,
                                          p_undefined=0.2), (np.arange(40, dtype=np.int64) * 10).astype(np.int32), 10, 20, 16


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def main():
    out = {}
    graphs = {}
    for name, g, seeds, T, top_n, G in cases():
        if id(g) not in graphs:
            graphs[id(g)] = FlatGraph(**g)
        F = graphs[id(g)]
        H = amd.Graph.from_flat(**g, tile_seeds=G)
        H.buildGraph()
        rec = amd.Recommender(H)
        ids, sc, cnt = rec.RecommendationBatch(seeds, 0.15, T, top_n)
        st = H.stats()
        oi, os_, oc = F.recommend_batch(seeds, 0.15, T, top_n)
        assert (cnt == oc).all(), (name, "counts differ from the oracle", cnt, oc)
        assert (ids == oi).all(), (name, "ids differ from the oracle")
        assert (bits(sc) == bits(os_)).all(), (name, "scores not bitwise equal to the oracle")
        if name.startswith("tie-G"):
            # the case is what it says: for some seed the cut at top_n passes through a group of equal scores
            _, o2, c2 = F.recommend_batch(seeds, 0.15, T, top_n + 1)
            assert ((c2 > top_n) & (bits(o2[:, top_n - 1]) == bits(o2[:, top_n]))).any(), (name, "no tie across the cut")
        out[name + "/ids"], out[name + "/scores"], out[name + "/counts"] = ids, bits(sc), cnt
        out[name + "/fused"] = np.array([st["rank_fused_groups"], st["rank_fused_fallbacks"]], dtype=np.int64)
        H.close()
    # a negative weight: the batched Recommendation refuses the graph, with or without the split
    g, _ = tie_graph()
    g["w"] = g["w"].copy()
    g["w"][3] = -1.0
    H = amd.Graph.from_flat(**g, tile_seeds=8)
    H.buildGraph()
    try:
        amd.Recommender(H).RecommendationBatch(np.arange(9, dtype=np.int32), 0.15, 10, 5)
        raise AssertionError("a graph with a negative weight was ranked")
    except _lib.RwrError as e:
        assert e.status == _lib.RWR_E_UNSUPPORTED
    out["negative/fused"] = np.array([H.stats()["rank_fused_groups"], H.stats()["rank_fused_fallbacks"]], dtype=np.int64)
    np.savez(sys.argv[1], **out)
    print("RANK_FUSED_CHILD_OK", len(out))


if __name__ == "__main__":
    main()
