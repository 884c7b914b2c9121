"""Model with a caller-set restart vector (the public field Model.restart, Model.cs:12): rwr_model_run_restart /
rwr_model_deliver_restart through the Python mirror, against the literal oracle (oracle/rwr_oracle.py Model) with the
same restart vector.  At most RWR_RESTART_EXACT_MAX non-zero entries: every rank bit is the oracle's; more: tolerance
parity, as the global model."""
import ctypes as C

import numpy as np
import pytest

from oracle import rwr_oracle as po
from tests import graphgen as gg

pytestmark = pytest.mark.gpu

EXACT_MAX = 256


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def amd():
    import recommendersystems_amd as amd
    from recommendersystems_amd import _lib
    assert _lib.load().rwr_device_count() >= 1, "no gfx950 device: the HIP path cannot run"
    return amd


def _graphs(amd, g):
    nodes, edges = po.from_flat(g["node_id"], g["node_type"], g["rowptr"], g["dst"], g["etype"], g["w"])
    PG = po.Graph(nodes, edges)
    PG.buildGraph()
    G = amd.Graph.from_flat(**g)
    G.buildGraph()
    return PG, G


# ~300 nodes: users, items, ETC users (dangling rows that only receive MENTION links), relabelled links
CASE = dict(seed=31, n_users=90, n_items=190, n_likes=1500, n_etc=20, n_friend=120, n_mention=150, n_author=40)


@pytest.fixture(scope="module")
def small(amd):
    g = gg.random_graph(**CASE)
    PG, G = _graphs(amd, g)
    n = len(g["node_id"])
    indeg = np.bincount(g["dst"][g["etype"] != 0], minlength=n)
    dangling = np.array([PG.graph[i] is None for i in range(n)])
    return g, PG, G, n, indeg, dangling


def _oracle_model(PG, d, seed, v, rank=None):
    """oracle Model with restart = v; restart loops over v's support only (bit-identical to the dense loops for finite
    ranks, tests/test_oracle.py)"""
    m = po.Model(PG, d, seed, dense_restart=False)
    m.restart = [float(x) for x in v]
    m._restart_nz = [r for r in range(len(v)) if v[r] != 0.0]
    if rank is not None:
        m.rank = [float(x) for x in rank]
    return m


def _supports(n, indeg, dangling):
    """support sets of 0, 1, 2, 8 and 256 rows: a dangling row, a row without in-links, the hub row among them"""
    rng = np.random.default_rng(7)
    hub = int(np.argmax(indeg))
    dang = int(np.flatnonzero(dangling & (indeg > 0))[0])
    noin = int(np.flatnonzero(indeg == 0)[0])
    rest = [int(x) for x in rng.permutation(n) if x not in (hub, dang, noin)]
    return {0: [], 1: [hub], 2: [dang, noin], 8: [hub, dang, noin] + rest[:5],
            256: [hub, dang, noin] + rest[:253]}


def _weights(k, rng):
    """many binades (1e-300 .. 1e3), both signs, no particular sum"""
    mag = 10.0 ** rng.uniform(-300, 3, size=k)
    mag[: min(k, 3)] = [1e3, 0.37, 1e-300][: min(k, 3)]
    sign = np.where(rng.random(k) < 0.3, -1.0, 1.0)
    return mag * sign


@pytest.mark.parametrize("d", [0.0, 0.15, 0.5, 1.0])
def test_sparse_restart_run_bitwise(amd, small, d):
    g, PG, G, n, indeg, dangling = small
    rng = np.random.default_rng(int(d * 100) + 1)
    for k, rows in _supports(n, indeg, dangling).items():
        v = np.zeros(n)
        v[rows] = _weights(len(rows), rng)
        for seed in (None, 5):
            m = _oracle_model(PG, d, seed, v)
            snap = {0: np.array(m.rank)}
            for t in range(1, 11):
                m.deliverRanks(); m.updateRanks()
                snap[t] = np.array(m.rank)
            for T in (0, 1, 2, 5, 10):
                dm = amd.Model(G, d) if seed is None else amd.Model(G, d, seed)
                dm.restart = v.copy()
                dm.run(T)
                assert (bits(dm.rank) == bits(snap[T])).all(), (k, seed, T)
                assert not dm.nextRank.any()


def _oracle_run_threshold(m, arg, cap=5000):
    """the oracle's run(double) / run() loop (Model.cs:52-66), statement for statement, with a cap on the steps"""
    threshold = (1 / 1.7976931348623157e308) * m.nNodes if arg is None else arg
    it = 0
    while True:
        m.deliverRanks()
        it += 1
        done = m.checkConvergence(threshold)
        m.updateRanks()
        if done:
            return it
        assert it < cap, "the oracle does not converge on this case"


# (support size, d, runs as (constructor seed, run argument)); run() only where the oracle reaches a fixed point (from
# the global state a one-row support ends in a cycle of last-bit changes, in the reference as in the oracle)
THRESHOLD_CASES = [(1, 0.15, ((None, 1e-10), (3, 1e-10), (3, None))),
                   (8, 0.15, ((None, 1e-10), (3, 1e-10), (None, None), (3, None))),
                   (256, 0.5, ((None, 1e-10), (3, 1e-10)))]


@pytest.mark.parametrize("k,d,runs", THRESHOLD_CASES, ids=lambda c: str(c) if isinstance(c, int) else None)
def test_sparse_restart_threshold_runs_bitwise(amd, small, k, d, runs):
    """run(1e-10) and run() (threshold (1/double.MaxValue) * n, Model.cs:53): same ranks, same iteration count -- the
    convergence sum is the reference's sequential one, bit for bit"""
    g, PG, G, n, indeg, dangling = small
    rng = np.random.default_rng(k)
    rows = _supports(n, indeg, dangling)[k]
    v = np.zeros(n)
    w = 10.0 ** rng.uniform(-300, 0, size=k)
    v[rows] = w / w.sum()
    for seed, arg in runs:
        m = _oracle_model(PG, d, seed, v)
        it = _oracle_run_threshold(m, arg)
        dm = amd.Model(G, d) if seed is None else amd.Model(G, d, seed)
        dm.restart = v.copy()
        dm.run(arg)
        assert dm.iterations == it, (seed, arg)
        assert (bits(dm.rank) == bits(m.rank)).all(), (seed, arg)


def test_dense_loops_agree_on_a_small_graph(amd):
    """the literal O(n^2) restart loops (dense_restart=True) on a small graph: edited restart incl. -0.0 entries"""
    g = gg.random_graph(5, n_users=30, n_items=70, n_likes=400, n_etc=6, n_friend=30, n_mention=40, n_author=10)
    PG, G = _graphs(amd, g)
    n = len(g["node_id"])
    v = np.zeros(n)
    v[[0, 17, 40, 99, n - 1]] = [0.25, -3.5, 1e-200, 7.0, 0.125]
    v[[3, 50]] = -0.0
    m = po.Model(PG, 0.3, 17, dense_restart=True)
    m.restart = list(v)
    m.run(5)
    dm = amd.Model(G, 0.3, 17)
    dm.restart = v.copy()
    dm.run(5)
    assert (bits(dm.rank) == bits(m.rank)).all()


def test_step_by_step_negative_ranks_bitwise(amd, small):
    """deliverRanks() / updateRanks() with an edited restart on a rank vector with negative entries"""
    g, PG, G, n, indeg, dangling = small
    rng = np.random.default_rng(3)
    sup = _supports(n, indeg, dangling)
    for k in (8, 256):
        v = np.zeros(n)
        v[sup[k]] = _weights(k, rng)
        x0 = rng.standard_normal(n) * 10.0 ** rng.uniform(-5, 5, size=n)
        m = _oracle_model(PG, 0.15, 0, v, rank=x0)
        dm = amd.Model(G, 0.15, 0)
        dm.restart = v.copy()
        dm.rank = x0.copy()
        for step in range(3):
            m.deliverRanks()
            dm.deliverRanks()
            assert (bits(dm.nextRank) == bits(m.nextRank)).all(), (k, step)
            m.updateRanks()
            dm.updateRanks()
        dm.run(2)                                  # run() continues from the current (negative-entry) rank
        m.run(2)
        assert (bits(dm.rank) == bits(m.rank)).all(), k


def _run_restart(amd, G, v, x, d, mode, value):
    from recommendersystems_amd import _lib
    lib = _lib.load()
    v = np.ascontiguousarray(v, dtype=np.float64)
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty_like(x)
    it = C.c_int64(0)
    st = lib.rwr_model_run_restart(G._handle(), v.ctypes.data_as(C.POINTER(C.c_double)),
                                   x.ctypes.data_as(C.POINTER(C.c_double)), d, mode, value,
                                   out.ctypes.data_as(C.POINTER(C.c_double)), C.byref(it))
    return st, out, int(it.value)


def test_cross_check_against_shipped_paths(amd, small):
    """restart = e_s on the personalised state is bitwise rwr_model_run(seed = s); restart = 1/n on the global state
    matches rwr_model_run(seed = -1) within 1e-12 relative"""
    from recommendersystems_amd import _lib
    g, PG, G, n, indeg, dangling = small
    for s in (0, int(np.argmax(indeg)), n - 1):
        e = np.zeros(n); e[s] = 1.0
        x = np.zeros(n); x[s] = float(n)
        for mode, value in ((_lib.RWR_RUN_ITERATIONS, 10.0), (_lib.RWR_RUN_THRESHOLD, 1e-10)):
            st, got, it = _run_restart(amd, G, e, x, 0.15, mode, value)
            assert st == _lib.RWR_OK
            ref = amd.Model(G, 0.15, s)
            ref.run(10 if mode == _lib.RWR_RUN_ITERATIONS else 1e-10)
            assert (bits(got) == bits(ref.rank)).all(), (s, mode)
            assert it == ref.iterations
    st, got, _ = _run_restart(amd, G, np.full(n, 1.0 / n), np.ones(n), 0.15, _lib.RWR_RUN_ITERATIONS, 10.0)
    assert st == _lib.RWR_OK
    ref = amd.Model(G, 0.15)
    ref.run(10)
    assert np.abs(got - ref.rank).max() <= 1e-12 * np.abs(ref.rank).max()


def test_dense_restart_tolerance(amd, small):
    """more than RWR_RESTART_EXACT_MAX non-zero entries: link-only SpMV + tree-summed mass * v[r]"""
    g, PG, G, n, indeg, dangling = small
    rng = np.random.default_rng(11)
    v = rng.random(n) + 1e-3
    v /= v.sum()
    assert np.count_nonzero(v) > EXACT_MAX
    for T in (1, 4, 10):
        m = _oracle_model(PG, 0.15, 2, v)
        m.run(T)
        dm = amd.Model(G, 0.15, 2)
        dm.restart = v.copy()
        dm.run(T)
        r = np.array(m.rank)
        assert np.abs(dm.rank - r).max() <= 1e-12 * np.abs(r).max(), T
    m = _oracle_model(PG, 0.5, None, v)
    it = _oracle_run_threshold(m, 1e-10)
    dm = amd.Model(G, 0.5)
    dm.restart = v.copy()
    dm.run(1e-10)
    assert abs(dm.iterations - it) <= 1
    assert np.abs(dm.rank - np.array(m.rank)).max() <= 1e-9


def test_larger_graph_multi_workgroup(amd):
    """~25 K nodes, |S| = 8: many fold rounds per chain, several waves in flight, the SpMV's row bins"""
    g = gg.random_graph(41, n_users=9000, n_items=15000, n_likes=120000, n_etc=500, n_friend=8000, n_mention=6000,
                        n_author=2000)
    PG, G = _graphs(amd, g)
    n = len(g["node_id"])
    indeg = np.bincount(g["dst"][g["etype"] != 0], minlength=n)
    rng = np.random.default_rng(2)
    rows = [int(np.argmax(indeg))] + [int(x) for x in rng.choice(n, 7, replace=False)]
    v = np.zeros(n)
    v[rows] = _weights(8, rng)
    m = _oracle_model(PG, 0.15, 100, v)
    dm = amd.Model(G, 0.15, 100)
    dm.restart = v.copy()
    for T in (1, 2):                                # 1 step, then 2 more from the advanced state
        m.run(T)
        dm.run(T)
        assert (bits(dm.rank) == bits(m.rank)).all(), T


def test_non_finite_restart_is_refused(amd, small):
    from recommendersystems_amd import _lib
    g, PG, G, n, indeg, dangling = small
    for bad in (np.inf, -np.inf, np.nan):
        v = np.zeros(n); v[4] = 0.5; v[9] = bad
        st, _, _ = _run_restart(amd, G, v, np.ones(n), 0.15, _lib.RWR_RUN_ITERATIONS, 3.0)
        assert st == _lib.RWR_E_UNSUPPORTED
        assert b"restart" in _lib.load().rwr_last_error()
        dm = amd.Model(G, 0.15, 1)
        dm.restart = v
        with pytest.raises(_lib.RwrError):
            dm.deliverRanks()
    x = np.ones(n); x[7] = np.inf
    v = np.zeros(n); v[4] = 0.5
    st, _, _ = _run_restart(amd, G, v, x, 0.15, _lib.RWR_RUN_ITERATIONS, 3.0)
    assert st == _lib.RWR_E_UNSUPPORTED
    # the graph stays usable
    m = _oracle_model(PG, 0.15, 1, v)
    m.run(3)
    dm = amd.Model(G, 0.15, 1)
    dm.restart = v.copy()
    dm.run(3)
    assert (bits(dm.rank) == bits(m.rank)).all()
