"""The chunked SpMM's index loads (recommendersystems_amd/csrc/spmm_chunk.h): a lane group loads up to 32
in-list entries at once, a long list's loads start on 128-byte lines of in_src, and the entries go out in gather rounds of
16.  None of that may move a bit of any result.

One explicit graph of 201 nodes whose in-list starts cover every residue mod 32 (rows of in-degree 0..31 in front: their
starts are the triangular numbers) and whose in-degrees include every boundary of a load, a round and the two-row wave
loop: 0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 97.  Two weightings: unit weights (the value-free kernels) and
unequal weights inside rows (the weighted kernels).  A batch of 40 seeds -- more than one tile, a padded one at 32 seeds per
tile, ITEM seeds (a seed-row chain in a tail step) and a seed without in-links among them -- at every tile width and at
iteration counts that reach the frontier-list, probing, dense and listed steps, against the C restatement of the reference:
ids, counts and score bits; then the whole rank matrix of a batch of Models, which covers the rows the ranking never reads."""
import numpy as np
import pytest

from tests import graphgen as gg

pytestmark = pytest.mark.gpu

DEGREES = list(range(32)) + [32, 33, 47, 48, 49, 63, 64, 65, 97]
N = 201
K = 40
TOP_N = 20
T_VALUES = (1, 2, 3, 6, 10)
TILE_SEEDS = (8, 16, 32, 64)
VARIANTS = ("unit", "weighted")


def make_graph(weighted: bool):
    rng = np.random.default_rng(20)
    indeg = np.array(DEGREES + list(rng.integers(1, 6, N - len(DEGREES))), dtype=np.int64)
    node_type = np.where(np.arange(N) % 3 == 1, gg.NODE_ITEM, gg.NODE_USER).astype(np.uint8)
    node_id = rng.permutation(np.arange(500, 500 + 3 * N, 3, dtype=np.int64))
    out = [[] for _ in range(N)]
    for j in range(N):
        others = np.delete(np.arange(N), j)
        for s in rng.choice(others, int(indeg[j]), replace=False):
            out[int(s)].append(j)
    rowptr = np.zeros(N + 1, dtype=np.int64)
    dst = []
    for i in range(N):
        dst += [out[i][t] for t in rng.permutation(len(out[i]))]
        rowptr[i + 1] = len(dst)
    dst = np.array(dst, dtype=np.int32)
    w = np.ones(len(dst), dtype=np.float64)
    if weighted:
        w = rng.integers(1, 9, len(dst)).astype(np.float64) * np.log(rng.integers(2, 40, len(dst))) / 7.3
    g = dict(node_id=node_id, node_type=node_type, rowptr=rowptr, dst=dst,
             etype=np.full(len(dst), gg.EDGE_LIKE, dtype=np.uint8), w=w)
    # the layout the test is about: what the transposed lists look like.  The library's in_ptr is indexed by node number with
    # no relabelling -- build.hip sorts the links stably by target and k_in_ptr counts them per target (DESIGN.md section 2,
    # the in_ptr / in_src row of the layout table); row_order only changes the order in which rows are walked -- and no link
    # is filtered here (none is UNDEFINED), so in_ptr[j] is the running sum of the in-degrees below
    got = np.bincount(dst, minlength=N)
    assert (got == indeg).all()
    starts = np.concatenate([[0], np.cumsum(got)])[:-1]
    assert set((starts[1:33] % 32).tolist()) == set(range(32))   # (row j starts at 0 + 1 + ... + (j - 1))
    assert {0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 97} <= set(got.tolist())
    return g


def seeds_for(g):
    s = np.arange(K, dtype=np.int32)   # node 0 has no in-link; every third node is an ITEM
    assert g["node_type"][s[0]] == gg.NODE_USER and (g["node_type"][s] == gg.NODE_ITEM).sum() >= 10
    return s


@pytest.fixture(scope="module")
def cases():
    from oracle.c_oracle import FlatGraph
    out = {}
    d32 = float(np.float32(0.15))
    for v in VARIANTS:
        g = make_graph(v == "weighted")
        F = FlatGraph(**g)
        seeds = seeds_for(g)
        lists = {T: F.recommend_batch(seeds, 0.15, T, TOP_N) for T in T_VALUES}
        ranks = np.stack([F.model_run(d32, int(s), 0, 6)[0] for s in seeds])
        out[v] = dict(g=g, seeds=seeds, lists=lists, ranks=ranks, d32=d32)
    return out


@pytest.mark.parametrize("tile_seeds", TILE_SEEDS)
@pytest.mark.parametrize("variant", VARIANTS)
def test_batch_lists_bitwise(variant, tile_seeds, cases):
    from recommendersystems_amd.rwr_based import Graph, Recommender
    c = cases[variant]
    G = Graph.from_flat(**c["g"], tile_seeds=tile_seeds)
    G.buildGraph()
    rec = Recommender(G)
    for T in T_VALUES:
        ids, sc, cnt = rec.RecommendationBatch(c["seeds"], 0.15, T, TOP_N)
        oi, os_, oc = c["lists"][T]
        assert (cnt == oc).all(), (variant, tile_seeds, T)
        assert (ids == oi).all(), (variant, tile_seeds, T)
        assert (sc.view(np.uint64) == os_.view(np.uint64)).all(), (variant, tile_seeds, T)
    st = G.stats()
    assert st["tile_seeds"] == tile_seeds
    assert st["uniform_path"] == (1 if variant == "unit" else 0)
    G.close()


@pytest.mark.parametrize("tile_seeds", TILE_SEEDS)
@pytest.mark.parametrize("variant", VARIANTS)
def test_model_batch_rank_matrix_bitwise(variant, tile_seeds, cases):
    from recommendersystems_amd.rwr_based import Graph, Model
    c = cases[variant]
    G = Graph.from_flat(**c["g"], tile_seeds=tile_seeds)
    G.buildGraph()
    ranks, iters = Model.RunBatch(G, c["d32"], c["seeds"], 6)
    assert (iters == 6).all()
    assert (ranks.view(np.uint64) == c["ranks"].view(np.uint64)).all(), (variant, tile_seeds)
    G.close()
