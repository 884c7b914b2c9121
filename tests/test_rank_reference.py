"""The NumPy ranking reference (tests/rank_reference.py) against both oracles, on the oracles' own rank vectors:
score and id bitwise equal at every position.  CPU only."""
import numpy as np
import pytest

from oracle import rwr_oracle as po
from oracle.c_oracle import FlatGraph
from tests import graphgen as gg
from tests.rank_reference import reference_ranking
from tests.test_gpu_parity import MEDIUM, SMALL

I64_MIN, I64_MAX = -(2 ** 63), 2 ** 63 - 1


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def full_range_ids(rng, n):
    """n unique int64 ids over the whole range, the two extremes and -1 / 0 / 1 included, shuffled."""
    fixed = np.array([I64_MIN, I64_MAX, -1, 0, 1, 2 ** 53 + 1, -(2 ** 53) - 1], dtype=np.int64)
    ids = set(int(x) for x in fixed[:n])
    while len(ids) < n:
        ids.add(int(rng.integers(I64_MIN, I64_MAX, dtype=np.int64, endpoint=True)))
    out = np.array(sorted(ids), dtype=np.int64)
    return out[rng.permutation(n)]


def with_full_range_ids(case, seed):
    g = gg.random_graph(**case)
    g["node_id"] = full_range_ids(np.random.default_rng(seed), len(g["node_id"]))
    return g


def item_seed_graph():
    """A seed that is itself an ITEM, LIKEs itself and LIKEs one item twice (Contains semantics)."""
    node_id = np.array([5, -3, 9, I64_MIN, I64_MAX, 0], dtype=np.int64)
    node_type = np.array([gg.NODE_USER, gg.NODE_ITEM, gg.NODE_ITEM, gg.NODE_ITEM, gg.NODE_ITEM, gg.NODE_ETC], dtype=np.uint8)
    lists = {0: [1, 2, 3], 1: [0, 1, 2, 2, 4], 2: [0, 1], 3: [0, 1], 4: [1, 5], 5: [4]}
    return gg._from_lists(node_id, node_type, lists)


CASES = ([("small", c, None) for c in SMALL] + [("medium", c, None) for c in MEDIUM]
         + [("fullrange", c, 100 + i) for i, c in enumerate(SMALL)]
         + [("fullrange", dict(seed=21, n_users=60, n_items=500, n_likes=700, n_friend=40), 7)])


def _graph(case, idseed):
    return gg.random_graph(**case) if idseed is None else with_full_range_ids(case, idseed)


@pytest.mark.parametrize("kind,case,idseed", CASES, ids=lambda v: v if isinstance(v, str) else (f"g{v['seed']}" if isinstance(v, dict) else str(v)))
def test_reference_matches_c_oracle(kind, case, idseed):
    g = _graph(case, idseed)
    F = FlatGraph(**g)
    n = len(g["node_id"])
    seeds = sorted({0, 1, case["n_users"] - 1, case["n_users"], n - 1})
    for T in (0, 1, 3, 10):
        for seed in seeds:
            for top_n in (0, 1, 7, 1024):
                oi, os_, rank = F.recommend(seed, 0.15, T, top_n, want_rank=True)
                ri, rs, rc = reference_ranking(rank, g["node_id"], g["node_type"], g["rowptr"], g["dst"], g["etype"], seed, top_n)
                assert rc == len(oi), (T, seed, top_n)
                assert (ri == oi).all(), (T, seed, top_n)
                assert (bits(rs) == bits(os_)).all(), (T, seed, top_n)


@pytest.mark.parametrize("kind,case,idseed", [c for c in CASES if c[1]["n_users"] + c[1]["n_items"] <= 600],
                         ids=lambda v: v if isinstance(v, str) else (f"g{v['seed']}" if isinstance(v, dict) else str(v)))
def test_reference_matches_literal_python_oracle(kind, case, idseed):
    g = _graph(case, idseed)
    nodes, edges = po.from_flat(g["node_id"], g["node_type"], g["rowptr"], g["dst"], g["etype"], g["w"])
    PG = po.Graph(nodes, edges)
    PG.buildGraph()
    n = len(g["node_id"])
    for T in (0, 1, 4):
        for seed in sorted({0, case["n_users"], n - 1}):
            m = po.Model(PG, po.widen_float(0.15), seed, dense_restart=False)
            m.run(T)
            rec = po.Recommender(PG, dense_restart=False).Recommendation(seed, 0.15, T)
            ri, rs, rc = reference_ranking(np.array(m.rank), g["node_id"], g["node_type"], g["rowptr"], g["dst"], g["etype"], seed)
            assert rc == len(rec)
            assert ri.tolist() == [r[0] for r in rec]
            assert (bits(rs) == bits([r[1] for r in rec])).all()


def test_reference_item_seed_and_duplicate_likes():
    g = item_seed_graph()
    F = FlatGraph(**g)
    nodes, edges = po.from_flat(g["node_id"], g["node_type"], g["rowptr"], g["dst"], g["etype"], g["w"])
    PG = po.Graph(nodes, edges)
    PG.buildGraph()
    for seed in range(len(g["node_id"])):
        for T in (0, 1, 2, 5):
            oi, os_, rank = F.recommend(seed, 0.15, T, 0, want_rank=True)
            ri, rs, rc = reference_ranking(rank, g["node_id"], g["node_type"], g["rowptr"], g["dst"], g["etype"], seed)
            rec = po.Recommender(PG).Recommendation(seed, 0.15, T)
            assert ri.tolist() == oi.tolist() == [r[0] for r in rec]
            assert (bits(rs) == bits(os_)).all() and (bits(rs) == bits([r[1] for r in rec])).all()
    # seed 1 is an ITEM that LIKEs itself: excluded; seed 2 is an ITEM that does not: a candidate of its own list
    _, _, rank = F.recommend(1, 0.15, 2, 0, want_rank=True)
    assert -3 not in reference_ranking(rank, g["node_id"], g["node_type"], g["rowptr"], g["dst"], g["etype"], 1)[0].tolist()
    _, _, rank = F.recommend(2, 0.15, 2, 0, want_rank=True)
    assert 9 in reference_ranking(rank, g["node_id"], g["node_type"], g["rowptr"], g["dst"], g["etype"], 2)[0].tolist()


def test_reference_ties_settle_by_id_over_the_full_range():
    """Equal scores (+0.0 and -0.0 compare equal, as double.CompareTo does) ordered by id descending over the whole int64
    range; the score bits are handed back untouched."""
    ids = np.array([0, I64_MIN, I64_MAX, -1, 1, 2 ** 53, -(2 ** 53)], dtype=np.int64)
    n = len(ids)
    node_type = np.full(n + 1, gg.NODE_ITEM, dtype=np.uint8)
    node_type[n] = gg.NODE_USER
    node_id = np.concatenate([ids, [77]]).astype(np.int64)
    rowptr = np.zeros(n + 2, dtype=np.int64)
    rank = np.array([0.0, -0.0, 0.0, 1.0, 0.0, -0.0, 0.0, 5.0])
    ri, rs, rc = reference_ranking(rank, node_id, node_type, rowptr, np.zeros(0, np.int32), np.zeros(0, np.uint8), n)
    assert rc == n
    assert ri.tolist() == [-1, I64_MAX, 2 ** 53, 1, 0, -(2 ** 53), I64_MIN]
    assert bits(rs).tolist() == bits([1.0, 0.0, -0.0, 0.0, 0.0, 0.0, -0.0]).tolist()
