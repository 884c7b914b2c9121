"""K personalised Models in one call (rwr_model_run_batch / Model.RunBatch).  Every row and iteration count
must be bitwise what rwr_model_run gives for that seed alone (Model(...).run(arg)), and a sample is checked against the C
restatement of the reference: iteration counts 0-10 at tile widths 1-64 over several tile groups, per-seed stopping in the
threshold modes, a handle whose buffers a ranked batch has left stale, the graphs and damping factors the ranked path
refuses, and the error cases."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle.c_oracle import FlatGraph
from tests import graphgen as gg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = float(np.float32(0.15))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def amd():
    import recommendersystems_amd as m
    from recommendersystems_amd import _lib
    assert _lib.load().rwr_device_count() >= 1, "no gfx950 device: the HIP path cannot run"
    return m


def graphs():
    """(name, flat graph): users, items, ETC nodes, UNDEFINED-relabelled links, dangling rows; weighted and uniform
    (the value-free matrix path); large enough that the G-wide sum scan runs its multi-block passes."""
    return [("weighted", gg.random_graph(21, n_users=1500, n_items=4000, n_likes=16000, n_etc=40, n_friend=400,
                                         n_mention=300, n_author=100)),
            ("uniform", gg.random_graph(22, n_users=1200, n_items=3500, n_likes=12000, n_etc=30, n_friend=300,
                                        n_author=80, uniform=True))]


def batch_seeds(g, K, rng):
    """K seeds with duplicates and dangling rows among them."""
    n = len(g["node_id"])
    dangling = np.flatnonzero(np.diff(g["rowptr"]) == 0)
    s = rng.integers(0, n, K).astype(np.int32)
    if K >= 4:
        s[1] = s[0]                                          # a duplicate
        s[-1] = dangling[0]                                  # dangling seeds
        s[K // 2] = dangling[-1]
        s[K // 3] = s[K // 2 + 1]                            # a duplicate in another tile
    return s


def singles(amd, G, seeds, arg, cache):
    """Per seed, what rwr_model_run alone gives (through Model(...).run(arg)); cached per (seed, arg)."""
    rows, its = [], []
    for s in seeds.tolist():
        key = (s, arg)
        if key not in cache:
            m = amd.Model(G, D, s)
            m.run(arg)
            cache[key] = (m.rank.copy(), m.iterations)
        rows.append(cache[key][0])
        its.append(cache[key][1])
    return np.array(rows), np.array(its, dtype=np.int64)


def same(got, want, what):
    ranks, iters = got
    wr, wi = want
    assert ranks.shape == wr.shape, what
    assert (iters == wi).all(), (what, "iteration counts", iters, wi)
    bad = np.flatnonzero((bits(ranks) != bits(wr)).any(axis=1))
    assert bad.size == 0, (what, "rows not bitwise equal", bad[:8])


def oracle_rows(F, seeds, mode, value, sample):
    out = {}
    for k in sample:
        out[k] = F.model_run(D, int(seeds[k]), mode, value)
    return out


@pytest.fixture(scope="module")
def setups(amd):
    out = []
    for name, g in graphs():
        Gref = amd.Graph.from_flat(**g)
        Gref.buildGraph()
        out.append((name, g, FlatGraph(**g), Gref, {}))
    yield out
    for *_, Gref, _ in out:
        Gref.close()


@pytest.mark.parametrize("tile_seeds", [1, 8, 16, 64])
def test_iteration_mode_bitwise(amd, setups, tile_seeds):
    from recommendersystems_amd import _lib
    for name, g, F, Gref, cache in setups:
        rng = np.random.default_rng(tile_seeds)
        K = 3 * tile_seeds + 1 if tile_seeds > 1 else 5
        seeds = batch_seeds(g, K, rng)
        G = amd.Graph.from_flat(**g, tile_seeds=tile_seeds, tile_group=1)   # several tile groups
        G.buildGraph()
        for T in (0, 1, 2, 3, 10):
            st0 = G.stats()
            got = amd.Model.RunBatch(G, D, seeds, T)
            st1 = G.stats()
            same(got, singles(amd, Gref, seeds, T, cache), (name, tile_seeds, T))
            for k, (r, it) in oracle_rows(F, seeds, _lib.RWR_RUN_ITERATIONS, T, (0, K // 2, K - 1)).items():
                assert it == T and (bits(got[0][k]) == bits(r)).all(), (name, tile_seeds, T, k, "oracle")
            assert st1["seeds_done"] == st0["seeds_done"], "a Model batch counted as ranked seeds"
            assert st1["spmm_seed_steps"] - st0["spmm_seed_steps"] == K * T
        G.close()


@pytest.mark.parametrize("threshold", [1e-3, 1e-9])
def test_threshold_modes_stop_per_seed(amd, setups, threshold):
    from recommendersystems_amd import _lib
    for name, g, F, Gref, cache in setups:
        seeds = batch_seeds(g, 37, np.random.default_rng(5))
        for tile_seeds in (0, 1, 8):
            G = amd.Graph.from_flat(**g, tile_seeds=tile_seeds)
            G.buildGraph()
            got = amd.Model.RunBatch(G, D, seeds, threshold)
            same(got, singles(amd, Gref, seeds, threshold, cache), (name, threshold, tile_seeds))
            # (the dangling seeds, which stop at step 1, already make the counts differ; that the other seeds stop at steps
            #  of their own too is shown by test_default_threshold, which asks for more than two distinct counts)
            assert len(set(got[1].tolist())) > 1, "every seed stopped at the same step: per-seed stopping not exercised"
            for k, (r, it) in oracle_rows(F, seeds, _lib.RWR_RUN_THRESHOLD, threshold, (2, 20, 36)).items():
                assert it == got[1][k] and (bits(got[0][k]) == bits(r)).all(), (name, threshold, k, "oracle")
            G.close()


def test_threshold_mode_over_several_tile_groups(amd):
    """Per-seed stopping with the batch spread over tile groups: 13 seeds in tiles of 4, one tile per group, so four groups
    run their own threshold loops (the last one a tile with one seed and three padding slots).  The contraction by 1 - d
    per step brings every seed below 1e-9 after a few hundred steps at the most; the dangling seed stops after step 1."""
    g = gg.random_graph(11, n_users=40, n_items=90, n_likes=400, n_etc=3, n_friend=20, n_mention=15)
    dangling = np.flatnonzero(np.diff(g["rowptr"]) == 0)
    seeds = np.array(list(range(12)) + [int(dangling[0])], dtype=np.int32)
    G = amd.Graph.from_flat(**g, tile_seeds=4, tile_group=1)
    G.buildGraph()
    got = amd.Model.RunBatch(G, D, seeds, 1e-9)
    st = G.stats()
    assert st["tile_seeds"] == 4 and st["tile_group"] == 1, "the batch did not run as four tile groups"
    same(got, singles(amd, G, seeds, 1e-9, {}), "several tile groups")
    assert got[1][-1] == 1 and len(set(got[1].tolist())) > 1
    G.close()


def test_default_threshold(amd):
    """run() (Model.cs:52-55): "until nothing changes", on a small graph where the reference converges for these seeds."""
    from recommendersystems_amd import _lib
    g = gg.random_graph(11, n_users=40, n_items=90, n_likes=400, n_etc=3, n_friend=20, n_mention=15)
    F = FlatGraph(**g)
    conv = [s for s in range(40) if F.model_run(D, s, _lib.RWR_RUN_DEFAULT_THRESHOLD, 0.0, max_iter=3000)[1] < 3000]
    dangling = np.flatnonzero(np.diff(g["rowptr"]) == 0)
    seeds = np.array(conv[:14] + [int(dangling[0]), conv[0]], dtype=np.int32)
    assert len(seeds) >= 10
    for tile_seeds in (0, 4, 16):
        G = amd.Graph.from_flat(**g, tile_seeds=tile_seeds)
        G.buildGraph()
        got = amd.Model.RunBatch(G, D, seeds)
        same(got, singles(amd, G, seeds, None, {}), ("default", tile_seeds))
        assert len(set(got[1].tolist())) > 2
        for k, s in enumerate(seeds.tolist()):
            r, it = F.model_run(D, s, _lib.RWR_RUN_DEFAULT_THRESHOLD, 0.0)
            assert it == got[1][k] and (bits(got[0][k]) == bits(r)).all(), ("default", k)
        G.close()


def test_reused_handle_after_ranked_batch(amd, setups):
    """A ranked batch (frontier-list steps, tail rows) leaves stale rows in X / Y / Z: the model batch must not see them."""
    for name, g, F, Gref, cache in setups:
        rng = np.random.default_rng(9)
        n = len(g["node_id"])
        seeds = batch_seeds(g, 24, rng)
        fresh = {}
        for arg in (1, 1e-3):
            G = amd.Graph.from_flat(**g, tile_seeds=16)
            G.buildGraph()
            fresh[arg] = amd.Model.RunBatch(G, D, seeds, arg)
            G.close()
        G = amd.Graph.from_flat(**g, tile_seeds=16)
        G.buildGraph()
        rec = amd.Recommender(G)
        for arg in (1, 1e-3):
            rec.RecommendationBatch(rng.integers(0, n, 40).astype(np.int32), D, 10, 20)
            assert G.stats()["frontier_list_launches"] > 0
            got = amd.Model.RunBatch(G, D, seeds, arg)
            same(got, fresh[arg], (name, "reused", arg))
            same(got, singles(amd, Gref, seeds, arg, cache), (name, "reused vs single", arg))
        G.close()


def test_domains_the_ranking_refuses(amd):
    """Negative raw weights (not `nonneg`) and d = 1.5: bitwise what rwr_model_run gives there (cases of
    test_negative_weights_take_the_general_path and test_error_paths_of_this_round)."""
    g = gg.random_graph(5, n_users=50, n_items=120, n_likes=700, n_friend=60, n_mention=50)
    w = g["w"].copy()
    rng = np.random.default_rng(3)
    pick = rng.choice(len(w), 40, replace=False)
    w[pick] = -0.25 * w[pick]
    g_neg = dict(g, w=w)
    g_d = gg.random_graph(5, n_users=50, n_items=200, n_likes=900, n_friend=40)
    for gname, gr, d, T in (("negative", g_neg, D, 6), ("d=1.5", g_d, 1.5, 4)):
        seeds = np.array([0, 7, 3, 0, 11, 42, 19, 8, 1, 2, 5, 9, 30, 31, 33, 40, 41], dtype=np.int32)
        for tile_seeds in (0, 16):
            G = amd.Graph.from_flat(**gr, tile_seeds=tile_seeds)
            G.buildGraph()
            ranks, iters = amd.Model.RunBatch(G, d, seeds, T)
            assert (iters == T).all()
            for k, s in enumerate(seeds.tolist()):
                m = amd.Model(G, d, s)
                m.run(T)
                assert (bits(ranks[k]) == bits(m.rank)).all(), (gname, tile_seeds, k)
            if gname == "d=1.5":
                r, _ = FlatGraph(**gr).model_run(1.5, 3, 0, T)
                assert (bits(ranks[2]) == bits(r)).all()
            G.close()


def test_errors(amd, setups):
    from recommendersystems_amd import _lib
    name, g, F, G, cache = setups[0]
    n = len(g["node_id"])
    for bad in (n, -1):
        with pytest.raises(amd.RwrError) as ei:
            amd.Model.RunBatch(G, D, np.array([0, 1, bad, 3], dtype=np.int32), 3)
        assert ei.value.status == _lib.RWR_E_RANGE and "batch position 2" in str(ei.value)
    ranks, iters = amd.Model.RunBatch(G, D, np.zeros(0, dtype=np.int32), 3)   # K = 0: a no-op
    assert ranks.shape == (0, n) and iters.shape == (0,)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "model_batch_child.py")], capture_output=True, text=True,
                       env=dict(os.environ, RWR_MAX_ITERS="20"), cwd=ROOT, timeout=600)
    assert p.returncode == 0 and "MODEL_BATCH_CHILD_OK" in p.stdout, f"{p.stdout[-3000:]}\n{p.stderr[-3000:]}"


def test_bad_arguments_with_a_handle(amd, setups):
    """K < 0 and an unknown run_mode on a valid handle are RWR_E_INVALID, before any device work (the no-GPU file can only
    pass a NULL handle, which is refused first)."""
    import ctypes as C
    from recommendersystems_amd import _lib
    lib = _lib.load()
    name, g, F, G, cache = setups[0]
    n = len(g["node_id"])
    seeds = np.array([0, 1], dtype=np.int32)
    out = np.full((2, n), 7.0)
    it = np.full(2, -5, dtype=np.int64)
    ps, po, pi = seeds.ctypes.data_as(C.POINTER(C.c_int32)), out.ctypes.data_as(C.POINTER(C.c_double)), \
        it.ctypes.data_as(C.POINTER(C.c_int64))
    assert lib.rwr_model_run_batch(G._handle(), ps, -1, D, _lib.RWR_RUN_ITERATIONS, 3.0, po, pi) == _lib.RWR_E_INVALID
    assert b"negative K" in lib.rwr_last_error()
    assert lib.rwr_model_run_batch(G._handle(), ps, 2, D, 7, 3.0, po, pi) == _lib.RWR_E_INVALID
    assert b"unknown run_mode 7" in lib.rwr_last_error()
    assert lib.rwr_model_run_batch(G._handle(), None, 2, D, _lib.RWR_RUN_ITERATIONS, 3.0, po, pi) == _lib.RWR_E_INVALID
    assert lib.rwr_model_run_batch(G._handle(), ps, 2, D, _lib.RWR_RUN_ITERATIONS, 3.0, None, pi) == _lib.RWR_E_INVALID
    assert (out == 7.0).all() and (it == -5).all(), "a refused call wrote results"
    assert lib.rwr_model_run_batch(G._handle(), ps, 2, D, _lib.RWR_RUN_ITERATIONS, 3.0, po, pi) == _lib.RWR_OK   # handle usable


def test_ranked_batch_after_model_batch(amd, setups):
    """A ranked batch after a model batch on one handle: the model batch's difference matrix is given back, and the ranked
    results are the oracle's."""
    name, g, F, G, cache = setups[0]
    n = len(g["node_id"])
    H = amd.Graph.from_flat(**g, tile_seeds=16)
    H.buildGraph()
    amd.Model.RunBatch(H, D, batch_seeds(g, 40, np.random.default_rng(2)), 1e-3)
    seeds = np.random.default_rng(4).integers(0, n, 40).astype(np.int32)
    bi, bs, bc = amd.Recommender(H).RecommendationBatch(seeds, D, 10, 20)
    oi, os_, oc = F.recommend_batch(seeds, D, 10, 20)
    assert (bc == oc).all() and (bi == oi).all() and (bits(bs) == bits(os_)).all()
    H.close()


def test_python_mirror_matches_single_models(amd, setups):
    name, g, F, G, cache = setups[1]
    seeds = batch_seeds(g, 19, np.random.default_rng(13))
    for arg in (4, 1e-6):
        ranks, iters = amd.Model.RunBatch(G, D, seeds, arg)
        for k, s in enumerate(seeds.tolist()):
            m = amd.Model(G, D, s)
            m.run(arg)
            assert m.iterations == iters[k] and (bits(m.rank) == bits(ranks[k])).all(), (arg, k)
