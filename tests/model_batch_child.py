"""Child process of tests/test_gpu_model_batch.py: librwr reads RWR_MAX_ITERS once per process, so the non-convergence
case runs here with a small limit.  Threshold 0.0 never satisfies diff < threshold (Model.cs:64): rwr_model_run_batch must
fail with RWR_E_UNSUPPORTED after RWR_MAX_ITERS steps, as rwr_model_run does, and a converging batch on the same handle
must still come back whole.  Prints MODEL_BATCH_CHILD_OK."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import graphgen as gg                        # noqa: E402


def main():
    import recommendersystems_amd as amd
    from recommendersystems_amd import _lib
    g = gg.random_graph(11, n_users=40, n_items=90, n_likes=400, n_etc=3, n_friend=20, n_mention=15)
    seeds = np.arange(0, 12, dtype=np.int32)
    # one tile group, then three (tiles of 4, one tile per group): the call fails at the first group that is stuck
    for opts in (dict(tile_seeds=8), dict(tile_seeds=4, tile_group=1)):
        G = amd.Graph.from_flat(**g, **opts)
        G.buildGraph()
        for call in (lambda: amd.Model.RunBatch(G, 0.15, seeds, 0.0), lambda: amd.Model(G, 0.15, 3).run(0.0)):
            try:
                call()
            except amd.RwrError as e:
                assert e.status == _lib.RWR_E_UNSUPPORTED and "RWR_MAX_ITERS" in str(e), str(e)
            else:
                raise AssertionError("a threshold of 0.0 converged")
        ranks, iters = amd.Model.RunBatch(G, 0.15, seeds, 1e30)   # every seed converges at step 1, far below the limit
        assert (iters == 1).all()
        for k in (5, 11):
            m = amd.Model(G, 0.15, int(seeds[k]))
            m.run(1)
            assert (ranks[k].view(np.uint64) == m.rank.view(np.uint64)).all()
        G.close()
    print("MODEL_BATCH_CHILD_OK")


if __name__ == "__main__":
    main()
