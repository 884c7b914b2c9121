"""Child process of tests/test_gpu_rank_head.py: librwr reads RWR_RANK_FUSED and RWR_RANK_FUSED_HEAD once per process, so
every head size runs in a fresh interpreter.  Runs every case below through RecommendationBatch (T = 6, top_n = 100), compares
ids, scores and counts bitwise with the C restatement of the reference, and writes them -- with the rank_fused_groups,
rank_fused_fallbacks and rank_pruned_rows counters of each call -- to the .npz named on the command line.

The graph: 300 users, 100 hot items liked by users 100..299 (60 fans each, drawn at random: in-degree 60, the highest by
far, so that they open tail_rows[0]) and N_COLD cold items with 6 000 random likes of all users.  The 40 seeds are users 0..39, who like cold items only: a head of the 100 hot rows gives every seed
exactly top_n entries and a positive threshold, a shorter head gives fewer and the threshold 0."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import recommendersystems_amd as amd                    # noqa: E402
from oracle.c_oracle import FlatGraph                   # noqa: E402
from tests.rank_fused_child import from_likes, bits     # noqa: E402

U, HOT, N_COLD = 300, 100, 7900
N_ITEMS = HOT + N_COLD
T, TOP_N = 6, 100


def graph():
    rng = np.random.default_rng(41)
    likes = []
    for j in range(HOT):
        likes += [(int(u), j) for u in rng.choice(np.arange(100, U), size=60, replace=False)]
    likes += [(int(u), HOT + int(v)) for u, v in zip(rng.integers(0, U, 6000), rng.integers(0, N_COLD, 6000))]
    likes += [(u, HOT + u) for u in range(40)]           # no seed is dangling
    return from_likes(U, N_ITEMS, likes)


def cases():
    """(name, seeds, tile_seeds): 40 seeds are two tiles at G = 32 and five at G = 8; 36 leave padded slots at both"""
    seeds = np.arange(40, dtype=np.int32)
    yield "G32", seeds, 32
    yield "G8", seeds, 8
    yield "G8-padded", seeds[:36], 8


def main():
    g = graph()
    F = FlatGraph(**g)
    out = {}
    for name, seeds, G in cases():
        H = amd.Graph.from_flat(**g, tile_seeds=G)
        H.buildGraph()
        ids, sc, cnt = amd.Recommender(H).RecommendationBatch(seeds, 0.15, T, TOP_N)
        st = H.stats()
        oi, os_, oc = F.recommend_batch(seeds, 0.15, T, TOP_N)
        assert (cnt == oc).all(), (name, "counts differ from the oracle", cnt, oc)
        assert (ids == oi).all(), (name, "ids differ from the oracle")
        assert (bits(sc) == bits(os_)).all(), (name, "scores not bitwise equal to the oracle")
        assert (cnt == TOP_N).all(), (name, "a seed reaches fewer than top_n items: the case is not what it says")
        out[name + "/ids"], out[name + "/scores"], out[name + "/counts"] = ids, bits(sc), cnt
        out[name + "/stats"] = np.array([st["rank_fused_groups"], st["rank_fused_fallbacks"], st["rank_pruned_rows"]],
                                        dtype=np.int64)
        print(name, out[name + "/stats"].tolist(), flush=True)
        H.close()
    np.savez(sys.argv[1], **out)
    print("RANK_HEAD_CHILD_OK", len(out))


if __name__ == "__main__":
    main()
