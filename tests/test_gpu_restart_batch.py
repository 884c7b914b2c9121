"""K Models with caller-set restart vectors in one call (rwr_model_run_restart_batch / Model.RunRestartBatch).
Every row and iteration count must be bitwise the literal oracle's (oracle/rwr_oracle.py Model with the sparse-restart idiom
of tests/test_gpu_restart.py) and bitwise what rwr_model_run_restart gives for that vector alone: iteration counts 0-10 at
tile widths 1-64, a larger graph with many fold rounds, per-vector stopping in the threshold modes, the reduction to
rwr_model_run_batch, the fallback classes, a handle whose buffers a ranked batch has left stale, and the error cases."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import rwr_oracle as po
from tests import graphgen as gg
from tests import restart_batch_child as rbc
from tests.restart_batch_child import bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT_MAX = 256


@pytest.fixture(scope="module")
def amd():
    import recommendersystems_amd as m
    from recommendersystems_amd import _lib
    assert _lib.load().rwr_device_count() >= 1, "no gfx950 device: the HIP path cannot run"
    return m


def _oracle_graph(g):
    nodes, edges = po.from_flat(g["node_id"], g["node_type"], g["rowptr"], g["dst"], g["etype"], g["w"])
    PG = po.Graph(nodes, edges)
    PG.buildGraph()
    return PG


def _oracle_model(PG, d, start, idx, val):
    """oracle Model with the given sparse restart vector (tests/test_gpu_restart.py: _oracle_model)"""
    n = len(PG.graph)
    m = po.Model(PG, d, None if start < 0 else int(start), dense_restart=False)
    v = [0.0] * n
    for i, x in zip(idx, val):
        v[int(i)] = float(x)
    m.restart = v
    m._restart_nz = [r for r in range(n) if v[r] != 0.0]
    return m


def _oracle_run_threshold(m, arg, cap=5000):
    """the oracle's run(double) / run() loop (Model.cs:52-66); None when it does not converge within cap steps"""
    threshold = (1 / 1.7976931348623157e308) * m.nNodes if arg is None else arg
    it = 0
    while it < cap:
        m.deliverRanks()
        it += 1
        done = m.checkConvergence(threshold)
        m.updateRanks()
        if done:
            return it
    return None


def _dense(n, idx, val):
    v = np.zeros(n)
    v[np.asarray(idx, dtype=np.int64)] = val
    return v


def _rank0(n, start):
    x = np.ones(n) if start < 0 else np.zeros(n)
    if start >= 0:
        x[start] = float(n)
    return x


def _single(G, n, idx, val, start, d, mode, value):
    """rwr_model_run_restart for one vector: (status, rank, iterations)"""
    from recommendersystems_amd import _lib
    lib = _lib.load()
    v, x = _dense(n, idx, val), _rank0(n, start)
    out = np.empty(n)
    it = C.c_int64(0)
    P = C.POINTER(C.c_double)
    st = lib.rwr_model_run_restart(G._handle(), v.ctypes.data_as(P), x.ctypes.data_as(P), d, mode, value, out.ctypes.data_as(P),
                                   C.byref(it))
    return st, out, int(it.value)


def _mode(arg):
    from recommendersystems_amd import _lib
    if isinstance(arg, int):
        return _lib.RWR_RUN_ITERATIONS, float(arg)
    return (_lib.RWR_RUN_DEFAULT_THRESHOLD, 0.0) if arg is None else (_lib.RWR_RUN_THRESHOLD, float(arg))


def _same_as_singles(amd, G, n, restarts, starts, d, arg, what, Gsingle=None):
    from recommendersystems_amd import _lib
    ranks, iters = amd.Model.RunRestartBatch(G, d, restarts, starts, arg)
    mode, value = _mode(arg)
    for k, (idx, val) in enumerate(restarts):
        st, r, it = _single(Gsingle or G, n, idx, val, -1 if starts is None else int(starts[k]), d, mode, value)
        assert st == _lib.RWR_OK
        assert it == iters[k], (what, k, "iterations", it, iters[k])
        assert (bits(r) == bits(ranks[k])).all(), (what, k, "row not bitwise the single call's")
    return ranks, iters


@pytest.fixture(scope="module")
def case(amd):
    g, n, indeg, dangling = rbc.case_graph()
    restarts, starts = rbc.case_vectors(n, indeg, dangling)
    PG = _oracle_graph(g)
    assert [len(i) for i, _ in restarts] == list(rbc.SIZES) and len(restarts) == 19
    assert PG.graph[int(starts[3])] is None                      # a dangling start
    snapshots = {}
    for di, d in enumerate(rbc.DS):
        rows = {T: [] for T in rbc.TS}
        for (idx, val), s in zip(restarts, starts):
            m = _oracle_model(PG, d, int(s), idx, val)
            for t in range(0, max(rbc.TS) + 1):
                if t in rows:
                    rows[t].append(np.array(m.rank))
                m.deliverRanks(); m.updateRanks()
        for T in rbc.TS:
            snapshots[(di, T)] = bits(np.array(rows[T]))
    G = amd.Graph.from_flat(**g)
    G.buildGraph()
    yield g, n, indeg, dangling, restarts, starts, PG, snapshots, G
    G.close()


def _case1_still_right(amd, case):
    """the handle still answers case 1 (d = 0.15, T = 5)"""
    g, n, indeg, dangling, restarts, starts, PG, snapshots, G = case
    ranks, iters = amd.Model.RunRestartBatch(G, 0.15, restarts, starts, 5)
    assert (iters == 5).all() and (bits(ranks) == snapshots[(1, 5)]).all()


def test_bitwise_against_the_oracle(amd, case):
    """case 1: one batch of 19 vectors at every d, T and tile width"""
    g, n, indeg, dangling, restarts, starts, PG, snapshots, G = case
    rbc.run_case1(amd, g, restarts, starts, snapshots)


def test_larger_graph_against_single_calls(amd):
    """~25 K nodes (tests/test_gpu_restart.py: test_larger_graph_multi_workgroup), K = 12 with |S| = 8: many fold rounds per
    chain, the strided column reads, chains of several tiles resident at once"""
    g = gg.random_graph(41, n_users=9000, n_items=15000, n_likes=120000, n_etc=500, n_friend=8000, n_mention=6000,
                        n_author=2000)
    n = len(g["node_id"])
    indeg = np.bincount(g["dst"][g["etype"] != 0], minlength=n)
    rng = np.random.default_rng(2)
    hub = int(np.argmax(indeg))
    restarts = []
    for k in range(12):
        rows = rng.choice(n, 8, replace=False).astype(np.int32)
        restarts.append((rows, np.abs(rng.standard_normal(8)) + 0.01))
    restarts[3][0][0] = hub                                        # one vector contains the hub
    restarts[5][0][2] = restarts[4][0][6]                          # two vectors share a support row
    restarts[9] = (restarts[8][0].copy(), restarts[8][1].copy())   # two vectors are identical
    for idx, _ in restarts:
        assert len(set(idx.tolist())) == 8
    starts = np.array([100, -1, 7, -1, 100, 2000, -1, 9, 5, 5, -1, 12000], dtype=np.int32)
    G = amd.Graph.from_flat(**g)
    G.buildGraph()
    for T in (1, 3):
        ranks, _ = _same_as_singles(amd, G, n, restarts, starts, 0.15, T, ("larger", T))
        assert (bits(ranks[8]) == bits(ranks[9])).all()
    G.close()


def test_threshold_modes_stop_per_vector(amd, case):
    """the non-negative normalised vectors and (start, argument) pairs of tests/test_gpu_restart.py: THRESHOLD_CASES, those
    the oracle converges on, batched by (d, argument): per-vector iteration counts and ranks are the oracle's"""
    from recommendersystems_amd import _lib
    from tests.test_gpu_restart import THRESHOLD_CASES, _supports
    g, n, indeg, dangling, restarts, starts, PG, snapshots, G = case
    pdang = np.array([PG.graph[i] is None for i in range(n)])
    batches = {}
    for k, d, runs in THRESHOLD_CASES:
        rng = np.random.default_rng(k)
        rows = _supports(n, indeg, pdang)[k]
        w = 10.0 ** rng.uniform(-300, 0, size=k)
        for seed, arg in runs:
            batches.setdefault((d, arg), []).append((np.array(rows, dtype=np.int32), w / w.sum(), -1 if seed is None else seed))
    distinct = set()
    for (d, arg), vecs in batches.items():
        keep, want = [], []
        for idx, val, s in vecs:
            m = _oracle_model(PG, d, s, idx, val)
            it = _oracle_run_threshold(m, arg)
            if it is not None:
                keep.append((idx, val, s))
                want.append((it, np.array(m.rank)))
        assert len(keep) >= 2, (d, arg)
        rs, st = [(i, v) for i, v, _ in keep], np.array([s for _, _, s in keep], dtype=np.int32)
        for tile_seeds in (0, 1):
            H = amd.Graph.from_flat(**g, tile_seeds=tile_seeds)
            H.buildGraph()
            ranks, iters = amd.Model.RunRestartBatch(H, d, rs, st, arg)
            H.close()
            print("threshold batch", d, arg, tile_seeds, iters.tolist(), [it for it, _ in want])
            for j, (it, r) in enumerate(want):
                assert iters[j] == it, (d, arg, j, iters[j], it)
                assert (bits(ranks[j]) == bits(r)).all(), (d, arg, j)
        distinct |= set(iters.tolist())
        if len(keep) >= 4:
            assert len(set(iters.tolist())) > 1, "every vector stopped at the same step: per-vector stopping not exercised"
    assert len(distinct) > 2
    # iters_out = NULL is accepted
    (d, arg), vecs = next(iter(batches.items()))
    lib = _lib.load()
    ptr = np.array([0, len(vecs[0][0]), len(vecs[0][0]) + len(vecs[1][0])], dtype=np.int64)
    idx = np.concatenate([vecs[0][0], vecs[1][0]]).astype(np.int32)
    val = np.concatenate([vecs[0][1], vecs[1][1]])
    out = np.zeros((2, n))
    mode, value = _mode(arg)
    st = lib.rwr_model_run_restart_batch(G._handle(), 2, ptr.ctypes.data_as(C.POINTER(C.c_int64)),
                                         idx.ctypes.data_as(C.POINTER(C.c_int32)), val.ctypes.data_as(C.POINTER(C.c_double)),
                                         None, d, mode, value, out.ctypes.data_as(C.POINTER(C.c_double)), None)
    assert st == _lib.RWR_OK
    both, _ = amd.Model.RunRestartBatch(G, d, [(vecs[0][0], vecs[0][1]), (vecs[1][0], vecs[1][1])], None, arg)
    assert (bits(out) == bits(both)).all()


def test_reduces_to_the_personalised_batch(amd, case):
    """restart {s: 1.0} with start = s is the personalised Model: rows and iteration counts of rwr_model_run_batch"""
    g, n, indeg, dangling, restarts, starts, PG, snapshots, G = case
    seeds = np.array([0, int(np.argmax(indeg)), n - 1, 5, 17, int(np.flatnonzero(dangling)[0]), 41], dtype=np.int32)
    rs = [{int(s): 1.0} for s in seeds]
    for arg in (10, 1e-10):
        ranks, iters = amd.Model.RunRestartBatch(G, 0.15, rs, seeds, arg)
        wr, wi = amd.Model.RunBatch(G, 0.15, seeds, arg)
        assert (iters == wi).all(), (arg, iters, wi)
        assert (bits(ranks) == bits(wr)).all(), arg


def test_fallbacks_equal_the_single_calls(amd, case):
    g, n, indeg, dangling, restarts, starts, PG, snapshots, G = case
    rng = np.random.default_rng(23)
    wide_rows = rng.choice(n, EXACT_MAX + 1, replace=False).astype(np.int32)
    wide = (wide_rows, rng.random(EXACT_MAX + 1) + 1e-3)
    rs = [restarts[3], wide, restarts[4], restarts[1]]
    st = np.array([-1, 2, 9, -1], dtype=np.int32)
    _same_as_singles(amd, G, n, rs, st, 0.15, 4, ("wide", 4))
    # a threshold run: non-negative vectors of sum 1 (the walk keeps its mass and converges; weights of both signs and sums
    # far from 1, as in case 1, need not)
    rs = [(i, np.abs(v) / np.abs(v).sum()) for i, v in rs]
    _same_as_singles(amd, G, n, rs, st, 0.15, 1e-6, ("wide", 1e-6))
    # a graph with negative weights, and d = 1.5 (tests/test_gpu_model_batch.py: test_domains_the_ranking_refuses)
    gb = gg.random_graph(5, n_users=50, n_items=120, n_likes=700, n_friend=60, n_mention=50)
    w = gb["w"].copy()
    pick = np.random.default_rng(3).choice(len(w), 40, replace=False)
    w[pick] = -0.25 * w[pick]
    g_neg = dict(gb, w=w)
    g_d = gg.random_graph(5, n_users=50, n_items=200, n_likes=900, n_friend=40)
    for gname, gr, d, T in (("negative", g_neg, 0.15, 6), ("d=1.5", g_d, 1.5, 4)):
        nn = len(gr["node_id"])
        vr = np.random.default_rng(8)
        rs = [(vr.choice(nn, k, replace=False).astype(np.int32), vr.random(k) + 0.1) for k in (1, 8, 3, 0, 20)]
        st = np.array([0, -1, 7, -1, 3], dtype=np.int32)
        for tile_seeds in (0, 16):
            H = amd.Graph.from_flat(**gr, tile_seeds=tile_seeds)
            H.buildGraph()
            _same_as_singles(amd, H, nn, rs, st, d, T, (gname, tile_seeds))
            H.close()
    # one vector: the single call
    _same_as_singles(amd, G, n, [restarts[4]], np.array([3], dtype=np.int32), 0.15, 5, "K=1")


def test_reused_handle_after_ranked_batch(amd):
    """A ranked batch (frontier-list steps, tail rows) leaves stale rows in X / Y: the restart batch must not see them."""
    g = gg.random_graph(21, n_users=1500, n_items=4000, n_likes=16000, n_etc=40, n_friend=400, n_mention=300, n_author=100)
    n = len(g["node_id"])
    rng = np.random.default_rng(9)
    rs = [(rng.choice(n, k, replace=False).astype(np.int32), rng.random(k) + 0.05) for k in (8, 1, 0, 3, 8, 64, 2, 8, 1, 5, 8, 8,
                                                                                              16, 1, 4, 8, 2, 8, 8, 3, 1)]
    rs = [(i, v / v.sum() if len(v) else v) for i, v in rs]       # sum 1: the threshold run below converges
    st = rng.integers(-1, n, len(rs)).astype(np.int32)
    fresh = {}
    for arg in (1, 3, 1e-3):
        G = amd.Graph.from_flat(**g, tile_seeds=16)
        G.buildGraph()
        fresh[arg] = amd.Model.RunRestartBatch(G, 0.15, rs, st, arg)
        G.close()
    G = amd.Graph.from_flat(**g, tile_seeds=16)
    G.buildGraph()
    rec = amd.Recommender(G)
    for arg in (1, 3, 1e-3):
        rec.RecommendationBatch(rng.integers(0, n, 40).astype(np.int32), 0.15, 10, 20)
        assert G.stats()["frontier_list_launches"] > 0
        ranks, iters = amd.Model.RunRestartBatch(G, 0.15, rs, st, arg)
        assert (iters == fresh[arg][1]).all(), arg
        assert (bits(ranks) == bits(fresh[arg][0])).all(), arg
    G.close()


def test_errors_on_a_live_graph(amd, case):
    from recommendersystems_amd import _lib
    g, n, indeg, dangling, restarts, starts, PG, snapshots, G = case
    ok = [({1: 0.5, 7: 0.25}), ({3: 1.0}), ({4: 2.0, 9: 1.0, 11: 0.5})]
    with pytest.raises(amd.RwrError) as ei:                           # the same index twice
        amd.Model.RunRestartBatch(G, 0.15, [ok[0], ([4, 9, 4], [1.0, 2.0, 3.0]), ok[2]], None, 3)
    assert ei.value.status == _lib.RWR_E_INVALID and "index 4" in str(ei.value) and "vector 1" in str(ei.value)
    _case1_still_right(amd, case)
    with pytest.raises(amd.RwrError) as ei:                           # an index of n
        amd.Model.RunRestartBatch(G, 0.15, [ok[0], ok[1], ([4, n], [1.0, 2.0])], None, 3)
    assert ei.value.status == _lib.RWR_E_RANGE and "batch position 2" in str(ei.value)
    _case1_still_right(amd, case)
    with pytest.raises(amd.RwrError) as ei:                           # a start of n
        amd.Model.RunRestartBatch(G, 0.15, ok, [0, n, -1], 3)
    assert ei.value.status == _lib.RWR_E_RANGE and "batch position 1" in str(ei.value)
    with pytest.raises(amd.RwrError) as ei:
        amd.Model.RunRestartBatch(G, 0.15, ok, [0, 1, -2], 3)
    assert ei.value.status == _lib.RWR_E_RANGE and "batch position 2" in str(ei.value)
    _case1_still_right(amd, case)
    for bad in (np.inf, -np.inf, np.nan):
        with pytest.raises(amd.RwrError) as ei:
            amd.Model.RunRestartBatch(G, 0.15, [ok[0], ([4, 9], [0.5, bad])], None, 3)
        assert ei.value.status == _lib.RWR_E_UNSUPPORTED and "restart" in str(ei.value)
    _case1_still_right(amd, case)
    # a +-0.0 entry is ignored: the result equals the batch without it
    with_zeros = [({1: 0.5, 30: -0.0, 7: 0.25, 2: 0.0}), ({3: 1.0, 0: -0.0}), ({40: 0.0})]
    without = [({1: 0.5, 7: 0.25}), ({3: 1.0}), ({})]
    for arg in (4, 1e-8):
        a = amd.Model.RunRestartBatch(G, 0.15, with_zeros, [2, -1, 5], arg)
        b = amd.Model.RunRestartBatch(G, 0.15, without, [2, -1, 5], arg)
        assert (a[1] == b[1]).all() and (bits(a[0]) == bits(b[0])).all()
    # K = 0: a no-op; bad arguments on a live handle write nothing
    ranks, iters = amd.Model.RunRestartBatch(G, 0.15, [], None, 3)
    assert ranks.shape == (0, n) and iters.shape == (0,)
    lib = _lib.load()
    ptr = np.array([0, 1, 2], dtype=np.int64)
    idx = np.array([1, 2], dtype=np.int32)
    val = np.array([1.0, 1.0])
    out = np.full((2, n), 7.0)
    it = np.full(2, -5, dtype=np.int64)
    pp, pi, pv = ptr.ctypes.data_as(C.POINTER(C.c_int64)), idx.ctypes.data_as(C.POINTER(C.c_int32)), \
        val.ctypes.data_as(C.POINTER(C.c_double))
    po_, pit = out.ctypes.data_as(C.POINTER(C.c_double)), it.ctypes.data_as(C.POINTER(C.c_int64))
    h, ITER = G._handle(), _lib.RWR_RUN_ITERATIONS
    call = lib.rwr_model_run_restart_batch
    assert call(h, -1, pp, pi, pv, None, 0.15, ITER, 3.0, po_, pit) == _lib.RWR_E_INVALID
    assert b"negative K" in lib.rwr_last_error()
    assert call(h, 2, pp, pi, pv, None, 0.15, 7, 3.0, po_, pit) == _lib.RWR_E_INVALID
    assert b"unknown run_mode 7" in lib.rwr_last_error()
    assert call(h, 2, None, pi, pv, None, 0.15, ITER, 3.0, po_, pit) == _lib.RWR_E_INVALID
    assert call(h, 2, pp, pi, pv, None, 0.15, ITER, 3.0, None, pit) == _lib.RWR_E_INVALID
    assert call(h, 2, pp, None, pv, None, 0.15, ITER, 3.0, po_, pit) == _lib.RWR_E_INVALID
    assert call(h, 2, pp, pi, None, None, 0.15, ITER, 3.0, po_, pit) == _lib.RWR_E_INVALID
    for bad_ptr in ([1, 1, 2], [0, 2, 1]):
        bp = np.array(bad_ptr, dtype=np.int64)
        assert call(h, 2, bp.ctypes.data_as(C.POINTER(C.c_int64)), pi, pv, None, 0.15, ITER, 3.0, po_, pit) == _lib.RWR_E_INVALID
        assert b"sup_ptr" in lib.rwr_last_error()
    assert (out == 7.0).all() and (it == -5).all(), "a refused call wrote results"
    zp = np.zeros(3, dtype=np.int64)                                 # empty supports, NULL index and value arrays: link-only walks
    assert call(h, 2, zp.ctypes.data_as(C.POINTER(C.c_int64)), None, None, None, 0.15, ITER, 3.0, po_, pit) == _lib.RWR_OK
    both, _ = amd.Model.RunRestartBatch(G, 0.15, [{}, {}], None, 3)
    assert (bits(out) == bits(both)).all() and (it == 3).all()
    _case1_still_right(amd, case)


@pytest.mark.parametrize("spmm", ["0", "1"])
def test_environment_selectors(amd, case, tmp_path, spmm):
    """RWR_SPMM chooses between the SpMM kernels the link-only step runs through: case 1 under each value in
    a fresh process; and, with a small RWR_MAX_ITERS, the non-convergence failure"""
    g, n, indeg, dangling, restarts, starts, PG, snapshots, G = case
    f = tmp_path / "snapshots.npz"
    np.savez(f, **{f"d{di}_T{T}": v for (di, T), v in snapshots.items()})
    child = os.path.join(ROOT, "tests", "restart_batch_child.py")
    p = subprocess.run([sys.executable, child, "case1", str(f)], capture_output=True, text=True,
                       env=dict(os.environ, RWR_SPMM=spmm), cwd=ROOT, timeout=600)
    assert p.returncode == 0 and "RESTART_BATCH_CHILD_OK" in p.stdout, f"{p.stdout[-3000:]}\n{p.stderr[-3000:]}"
    if spmm == "1":
        p = subprocess.run([sys.executable, child, "stuck"], capture_output=True, text=True,
                           env=dict(os.environ, RWR_MAX_ITERS="20"), cwd=ROOT, timeout=600)
        assert p.returncode == 0 and "RESTART_BATCH_CHILD_OK" in p.stdout, f"{p.stdout[-3000:]}\n{p.stderr[-3000:]}"
