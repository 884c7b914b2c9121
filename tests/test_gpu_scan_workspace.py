"""The binade scan's workspace (chain_scan.hip: cs_workspace_ensure) is shared by users of different geometry.  On ONE handle
(tile_seeds=8, seed_row_kernel="scan") four calls size it in turn -- Model.run with a threshold (chain_scan_sum: one slot at
G = 1, the smallest), Model.RunBatch with the same threshold (chain_scan_sum_cols at G = 8 over two tiles), a batched
Recommendation of the same 11 seeds (the steps' scan at G = 8) and a single-seed Recommendation (G = 1) -- first in this
order, growing the workspace, then in reverse on the buffers the larger calls have left.  The graph has 12 blocks of 1 024
rows at G = 1 (the single-seed block1 / carry1 form with its own sums) and 24 blocks of 512 rows at G = 8 (above the direct
walk's eight: the four-launch form).  Every result, the threshold runs' iteration counts included, must be bitwise the C
restatement's of the reference; nothing is compared with a second GPU handle."""
import numpy as np
import pytest

from oracle.c_oracle import FlatGraph
from tests import graphgen as gg

pytestmark = pytest.mark.gpu

D = float(np.float32(0.15))
THRESHOLD = 1e-3
T, TOP_N = 10, 20


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def case():
    """The graph, the 11 seeds (users; one twice) and the oracle's results, computed once."""
    from recommendersystems_amd import _lib
    g = gg.random_graph(31, n_users=4000, n_items=8000, n_likes=40000, n_etc=40, n_friend=900, n_mention=600, n_author=200)
    n = len(g["node_id"])
    assert -(-n // 1024) == 12 and -(-n * 8 // 4096) == 24, "the graph no longer has the block counts this test is about"
    seeds = np.random.default_rng(31).choice(4000, 11, replace=False).astype(np.int32)
    seeds[7] = seeds[2]
    F = FlatGraph(**g)
    runs = [F.model_run(D, int(s), _lib.RWR_RUN_THRESHOLD, THRESHOLD) for s in seeds]
    want = {
        "run": runs[0],
        "run_batch": (np.array([r for r, _ in runs]), np.array([it for _, it in runs], dtype=np.int64)),
        "batch": F.recommend_batch(seeds, 0.15, T, TOP_N),
        "single": F.recommend(int(seeds[3]), 0.15, T, TOP_N),
    }
    return g, seeds, want


def test_one_handle_across_scan_geometries(case):
    import recommendersystems_amd as amd
    from recommendersystems_amd import _lib
    assert _lib.load().rwr_device_count() >= 1, "no gfx950 device: the HIP path cannot run"
    g, seeds, want = case
    G = amd.Graph.from_flat(**g, tile_seeds=8, seed_row_kernel="scan")
    G.buildGraph()
    rec = amd.Recommender(G)

    def run():
        m = amd.Model(G, D, int(seeds[0]))
        m.run(THRESHOLD)
        rank, it = want["run"]
        assert m.iterations == it and (bits(m.rank) == bits(rank)).all(), "Model.run"

    def run_batch():
        ranks, iters = amd.Model.RunBatch(G, D, seeds, THRESHOLD)
        wr, wi = want["run_batch"]
        assert (iters == wi).all(), ("Model.RunBatch: iteration counts", iters, wi)
        assert (bits(ranks) == bits(wr)).all(), "Model.RunBatch: ranks"

    def batch():
        ids, sc, cnt = rec.RecommendationBatch(seeds, 0.15, T, TOP_N)
        oi, os_, oc = want["batch"]
        assert (cnt == oc).all() and (ids == oi).all() and (bits(sc) == bits(os_)).all(), "RecommendationBatch"

    def single():
        ids, sc = rec.RecommendationArrays(int(seeds[3]), 0.15, T, TOP_N)
        oi, os_ = want["single"]
        assert (np.asarray(ids) == oi).all() and (bits(sc) == bits(os_)).all(), "RecommendationArrays"

    calls = [run, run_batch, batch, single]
    for call in calls + calls[::-1]:
        call()
    assert len(set(want["run_batch"][1].tolist())) > 1, "every seed stopped at the same step"
    G.close()
