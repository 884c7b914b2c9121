"""The one candidate-list compaction (typed.hip's count / scan / scatter; cand_plan.h, filter_plan.h) through both of its
callers, at the node counts where its geometry changes: n = 1, CAND_BLOCK - 1, CAND_BLOCK, CAND_BLOCK + 1, and one n with
CAND_SCAN_CHUNK + 1 blocks, where the scan's carry crosses into a second trip and the last block holds one row.  Per n one
graph and one build of each list: the handle's cached list of a node type (rwr_recommend_typed_positions_batch) and a call's
own list (rwr_recommend_filtered_positions_batch: the same type under a pool of every node, and every type without a pool).
The positions entries answer for the WHOLE list, so asking for every node id reads the list back: an id is in it iff its
position is >= 0, and list_len is its length.  The expectation is the host model -- the rows of the type, which is what
filter_list() gives without a pool -- and the two builds must agree entry for entry, scores bitwise.

tests/test_gpu_typed.py::test_last_row_is_the_only_match and tests/test_gpu_filtered.py::test_block_and_word_edges already
run n = CAND_BLOCK and CAND_BLOCK + 1 through one caller each against the oracle; the other three shapes are only here."""
import numpy as np
import pytest

from tests import graphgen as gg
from tests.test_gpu_typed import bits, built

pytestmark = pytest.mark.gpu

D = 0.15
CAND_BLOCK = 256           # cand_plan.h
CAND_SCAN_CHUNK = 256      # cand_plan.h
WANTED = 200               # a node type of its own


@pytest.fixture(scope="module")
def amd():
    import recommendersystems_amd as m
    from recommendersystems_amd import _lib
    assert _lib.load().rwr_device_count() >= 1, "no gfx950 device: the HIP path cannot run"
    return m


def ring(n, types):
    """node i links to node (i + 1) % n; ids distinct and not the indices"""
    return dict(node_id=np.arange(n, dtype=np.int64) * 3 + 7, node_type=np.asarray(types, dtype=np.uint8),
                rowptr=np.arange(n + 1, dtype=np.int64), dst=((np.arange(n) + 1) % n).astype(np.int32),
                etype=np.full(n, gg.EDGE_LIKE, dtype=np.uint8), w=np.ones(n, dtype=np.float64))


@pytest.mark.parametrize("n", [1, CAND_BLOCK - 1, CAND_BLOCK, CAND_BLOCK + 1, CAND_SCAN_CHUNK * CAND_BLOCK + 1])
def test_both_lists_are_the_model(amd, n):
    rng = np.random.default_rng(n)
    types = np.where(rng.random(n) < 0.5, gg.NODE_USER, gg.NODE_ITEM).astype(np.uint8)
    if n <= CAND_BLOCK + 1:
        types[rng.random(n) < 0.4] = WANTED
    else:
        # few wanted rows (the positions entries count hits per slot): the first and last row of the blocks around both ends of
        # the scan's first trip, some anywhere, and the one row of the last block
        nb = CAND_SCAN_CHUNK + 1
        assert (n + CAND_BLOCK - 1) // CAND_BLOCK == nb
        for b in (0, 1, CAND_SCAN_CHUNK - 2, CAND_SCAN_CHUNK - 1):
            types[[b * CAND_BLOCK, b * CAND_BLOCK + CAND_BLOCK - 1]] = WANTED
        types[rng.choice(n, 200, replace=False)] = WANTED
    types[n - 1] = WANTED
    g = ring(n, types)
    model = np.flatnonzero(types == WANTED)                       # filter_list(node_type, n, WANTED, no bitmap)
    G = built(amd, g)
    rec = amd.Recommender(G)
    every = [g["node_id"]]
    cached = rec.RecommendationTypedPositionsBatch([0], D, 0, every, WANTED)
    again = rec.RecommendationTypedPositionsBatch([0], D, 0, every, WANTED)      # (the cached list, not built again)
    own = rec.RecommendationFilteredPositionsBatch([0], D, 0, every, WANTED, pool=np.arange(n))
    for what, (pos, sc, ln) in (("cached", cached), ("cached, second call", again), ("call-scoped", own)):
        print(what, n, "list_len", int(ln[0]), "model", model.size)
        assert int(ln[0]) == model.size, (what, n)
        assert np.flatnonzero(pos[0] >= 0).tolist() == model.tolist(), (what, n)
        assert sorted(pos[0][model].tolist()) == list(range(model.size)), (what, n, "positions are not a permutation")
        assert (pos[0] == cached[0][0]).all() and (bits(sc[0]) == bits(cached[1][0])).all(), (what, n, "the builds differ")
    # every type, no pool: the call-scoped build without a bitmap; 64 ids spread over the rows, the last one among them
    some = np.unique(np.concatenate([rng.choice(n, min(n, 63), replace=False), [n - 1]]))
    pos, _, ln = rec.RecommendationFilteredPositionsBatch([0], D, 0, [g["node_id"][some]], None)
    assert int(ln[0]) == n and (pos[0] >= 0).all() and len(set(pos[0].tolist())) == some.size, ("any type", n)
    G.close()
