"""Child process of tests/test_gpu_x_clear.py: librwr reads RWR_X_CLEAR, RWR_CHAIN and RWR_VALUE_FREE once per process, so every
setting runs in a fresh interpreter.  A ranking-only batch on the frontier-list path no longer clears its rank matrix (DESIGN
§3.3.2): whatever an earlier call left in the workspace stays in every row the first steps do not write, and the fold beside
step 2 reads step 1's output through the frontier bitmap.

One graph handle.  Per T: call 1 ranks the seed set `dirt` at T = 10, which leaves every row of both rank matrices non-zero;
call 2 ranks the disjoint set `seeds` at T and must equal the C restatement of the reference bit for bit.  With RWR_X_CLEAR=1
call 2 runs on a fresh handle instead (the cleared path, nothing stale).  Writes ids, scores, counts and the calls' counters
(x_clear_skipped, frontier_list_launches, chain_launches) to the .npz named on the command line.

The graph: tests/graphgen.py, 1 500 users, 2 500 items, likes only, unit weights, about six links per node (two act steps),
items without any link.  Two seed sets of 43 nodes at tile width 8, 42 of them live: six tiles, the last one padded.  Both hold
one user seven times -- seeds of equal in-degree are dealt to the six tiles in turn, so the first and the seventh copy share a
tile (two slots, one seed row) -- and a node without links.  "mixed" holds the node of most in-links, an ITEM row that step 2
reaches from rows inside and outside step 1's list: with an ITEM seed the group keeps every chain, step 1 lists whenever it is
not the last step, and at T = 3 the masked fold runs beside the LAST step.  "users" holds the user of most in-links instead:
without an ITEM seed the last steps walk the tail row lists, so step 1 is a tail-list step at T = 3 and 4 and lists at 6 and 10."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import recommendersystems_amd as amd                    # noqa: E402
from oracle.c_oracle import FlatGraph                   # noqa: E402
from tests import graphgen as gg                        # noqa: E402
from tests.tail_rows_child import bits                  # noqa: E402

T_VALUES = (2, 3, 4, 6, 10)
D = 0.15
TOP_N = 20
COUNTERS = ("x_clear_skipped", "frontier_list_launches", "chain_launches")


def graph_and_seeds():
    g = gg.random_graph(77, n_users=1500, n_items=2500, n_likes=12000, uniform=True)
    n = len(g["node_type"])
    assert len(g["dst"]) <= 64 * n                        # sparse: RWR_ACT_ITERS defaults to 2, so step 1 lists
    rng = np.random.default_rng(78)
    outdeg = np.diff(g["rowptr"])
    indeg = np.bincount(g["dst"][g["etype"] != gg.EDGE_UNDEFINED], minlength=n)
    is_user = g["node_type"] == gg.NODE_USER
    hub = int(np.argmax(indeg))
    assert g["node_type"][hub] == gg.NODE_ITEM
    hub_user = int(np.argmax(np.where(is_user, indeg, -1)))
    dangling = int(np.flatnonzero(outdeg == 0)[0])
    users = np.flatnonzero(is_user & (outdeg > 0))
    users = users[users != hub_user]
    pick = rng.choice(users, 80, replace=False)
    sets = {}
    for name, h in (("mixed", hub), ("users", hub_user)):
        sets[name] = np.concatenate([pick[:1].repeat(7), [h, dangling], pick[1:35]]).astype(np.int32)   # 43 slots
    dirt = pick[40:].astype(np.int32)
    assert all(len(s) == 43 and not set(s.tolist()) & set(dirt.tolist()) for s in sets.values())
    return g, sets, dirt


def main():
    fresh_handle = os.environ.get("RWR_X_CLEAR") == "1"
    g, sets, dirt = graph_and_seeds()
    F = FlatGraph(**g)
    out = {}
    H = None
    for name, seeds in sets.items():
        for T in T_VALUES:
            if H is None or fresh_handle:
                if H is not None:
                    H.close()
                H = amd.Graph.from_flat(**g, tile_seeds=8)
                H.buildGraph()
            rec = amd.Recommender(H)
            if not fresh_handle:
                rec.RecommendationBatch(dirt, D, 10, TOP_N)
            before = H.stats()
            ids, sc, cnt = rec.RecommendationBatch(seeds, D, T, TOP_N)
            after = H.stats()
            oi, os_, oc = F.recommend_batch(seeds, D, T, TOP_N)
            assert (cnt == oc).all(), (name, T, "counts differ from the oracle")
            assert (ids == oi).all(), (name, T, "ids differ from the oracle")
            assert (bits(sc) == bits(os_)).all(), (name, T, "scores not bitwise equal to the oracle")
            k = f"{name}/T{T}"
            out[k + "/ids"], out[k + "/scores"], out[k + "/counts"] = ids, bits(sc), cnt
            out[k + "/stats"] = np.array([after[c] - before[c] for c in COUNTERS], dtype=np.int64)
            print(k, out[k + "/stats"].tolist(), flush=True)
    H.close()
    np.savez(sys.argv[1], **out)
    print("X_CLEAR_CHILD_OK", len(out))


if __name__ == "__main__":
    main()
