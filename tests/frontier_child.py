"""Cases of tests/test_gpu_frontier.py, and its child process: batches whose first steps walk only each tile's frontier row
list and leave the other rows of Y / Z stale.  Every result is compared bit for bit with the C
restatement of the reference: tile widths 8-64, T = 1 .. 10, batches below and above the scan / fold threshold, several
tile groups sharing one workspace, ITEM / duplicate / dangling / hub seeds, graphs that are not bipartite and repeat links
to one target under several types; then stale buffers on one handle (a T = 10 batch, other seeds at T = 1 .. 4, a
Model.run full vector, a batch after rwr_graph_update_links).  librwr reads RWR_* once per process, so the test starts
this script with them set; it prints FRONTIER_CHILD_OK <cases> <frontier-list launches> <digest of every result>."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle.c_oracle import FlatGraph                   # noqa: E402
from tests import graphgen as gg                        # noqa: E402
from tests.tail_rows_child import bits, mixed_graph, retarget_item_links   # noqa: E402

T_VALUES = (1, 2, 3, 4, 5, 10)
TILE_WIDTHS = (8, 16, 32, 64)
D = 0.15


def seed_sets(g, rng):
    """(name, seeds): ITEM seeds among others, duplicates (inside one tile and across tiles), dangling rows, hubs."""
    nt, rp = g["node_type"], g["rowptr"]
    n = len(nt)
    outdeg = np.diff(rp)
    indeg = np.bincount(g["dst"], minlength=n)
    items = np.flatnonzero(nt == gg.NODE_ITEM)
    others = np.flatnonzero(nt != gg.NODE_ITEM)
    mixed = np.concatenate([rng.choice(items, 12, replace=False), rng.choice(others, 28, replace=False)])
    rng.shuffle(mixed)
    dup = rng.choice(others, 20, replace=False)
    dup = np.concatenate([dup, dup[:6], dup[:3]])        # a seed up to three times, in one tile and in others
    dangling = np.flatnonzero(outdeg == 0)
    dang = np.concatenate([dangling[:8], rng.choice(others, 16, replace=False)])
    hubs = np.concatenate([np.argsort(-indeg, kind="stable")[:10], np.argsort(-outdeg, kind="stable")[:10]])
    return [("mixed", mixed.astype(np.int32)), ("duplicates", dup.astype(np.int32)),
            ("dangling", dang.astype(np.int32)), ("hubs", hubs.astype(np.int32))]


def check(rec, F, seeds, T, what, h):
    bi, bs, bc = rec.RecommendationBatch(seeds, D, T, 20)
    oi, os_, oc = F.recommend_batch(seeds, D, T, 20)
    assert (bc == oc).all(), (what, "counts differ")
    assert (bi == oi).all(), (what, "ids differ")
    assert (bits(bs) == bits(os_)).all(), (what, "scores not bitwise equal")
    for a in (bi, bs, bc):
        h.update(np.ascontiguousarray(a).tobytes())


def run_all(amd):
    """Runs every case against the oracle; returns (cases, frontier-list launches, sha256 of all results)."""
    h = hashlib.sha256()
    cases = 0
    fl = 0
    for gname, gseed, uniform in (("weighted", 41, False), ("uniform", 42, True)):
        g = mixed_graph(gseed, uniform=uniform)
        n = len(g["node_type"])
        F = FlatGraph(**g)
        rng = np.random.default_rng(gseed)
        sets = seed_sets(g, rng)
        big = rng.integers(0, n, 700).astype(np.int32)   # above the binade scan's batch size: the fold chain
        for G_w in TILE_WIDTHS:
            mats = 4 if uniform else 2
            for wsname, ws in (("one-group", 0), ("groups", 3 * mats * n * G_w * 8)):
                G = amd.Graph.from_flat(**g, tile_seeds=G_w, workspace_bytes=ws)
                G.buildGraph()
                rec = amd.Recommender(G)
                for sname, seeds in sets:
                    for T in T_VALUES:
                        if ws and T not in (2, 3, 5):
                            continue
                        check(rec, F, seeds, T, (gname, G_w, wsname, sname, T), h)
                        cases += 1
                if G_w == 32 and not ws:
                    for T in (3, 4, 10):
                        check(rec, F, big, T, (gname, G_w, "big", T), h)
                        cases += 1
                fl += G.stats()["frontier_list_launches"]
                G.close()
        # stale buffers: one handle, a dense batch, then other seeds at short T, a single-seed full vector, a link update
        G = amd.Graph.from_flat(**g, tile_seeds=32)
        G.buildGraph()
        rec = amd.Recommender(G)
        check(rec, F, sets[0][1], 10, (gname, "stale", "dense"), h)
        for T in (1, 2, 3, 4):
            check(rec, F, sets[3][1], T, (gname, "stale", "after-dense", T), h)
            check(rec, F, sets[1][1], T, (gname, "stale", "after-dense-dup", T), h)
        seed = int(sets[0][1][0])
        m = amd.Model(G, float(np.float32(D)), seed)
        m.run(4)
        r, _ = F.model_run(float(np.float32(D)), seed, 0, 4)
        assert (bits(m.rank) == bits(r)).all(), (gname, "stale", "Model.run")
        h.update(bits(m.rank).tobytes())
        check(rec, F, sets[2][1], 3, (gname, "stale", "after-model"), h)
        g2, idx = retarget_item_links(g, rng)
        G.updateLinks(idx, etype=g2["etype"][idx], w=g2["w"][idx])
        F2 = FlatGraph(**g2)
        for T in (2, 3, 10):
            check(rec, F2, sets[0][1], T, (gname, "stale", "updated", T), h)
        cases += 14
        fl += G.stats()["frontier_list_launches"]
        G.close()
    return cases, fl, h.hexdigest()


def main():
    import recommendersystems_amd as amd
    cases, fl, digest = run_all(amd)
    print("FRONTIER_CHILD_OK", cases, fl, digest)


if __name__ == "__main__":
    main()
