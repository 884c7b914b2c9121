"""The arithmetic of the audience entry on the CPU (tests/audience_cases.py): the reverse recurrence against the literal forward
loop of Model.cs for EVERY (seed, target) pair of graphs of at most 150 nodes, within the derived tolerance, zeros on zeros;
and the restart-mass host model of audience_plan.h, through the compiled check program, bitwise against NumPy's."""
import struct
import subprocess

import numpy as np
import pytest

from tests import audience_cases as ac
from tests import graphgen as gg
from tests.test_audience_plan import build_check


def _graphs():
    yield "mixed", gg.random_graph(3, n_users=30, n_items=60, n_likes=260, n_etc=4, n_friend=20, n_mention=25, n_author=10)
    yield "uniform", gg.random_graph(4, n_users=25, n_items=50, n_likes=200, uniform=True)
    yield "half_dangling", ac.degree_graph([0, 1, 4, 5, 9, 0, 2, 0, 30, 3, 0, 7], 5, n_items=60)
    yield "no_dangling", ac.drop_dangling(gg.random_graph(6, n_users=20, n_items=40, n_likes=150, n_friend=10))
    yield "kat2", gg.kat2()


@pytest.mark.parametrize("T,d", [(0, 0.15), (1, 0.15), (3, 0.5), (4, 1.0), (5, 0.15), (10, float(np.float32(0.15)))])
def test_reverse_is_forward_for_every_pair(T, d):
    worst_all = 0.0
    for name, g in _graphs():
        n = len(g["rowptr"]) - 1
        assert n <= 150
        wn, nd = ac.normalise(g)
        F = ac.forward(g, wn, nd, np.arange(n), T, d)            # F[s, v]
        S = ac.reverse(g, wn, nd, np.arange(n), T, d)            # S[s, v]
        tol = ac.tol_rel(g, T, d)
        zero = F == 0.0
        assert (S[zero] == 0.0).all() and not np.signbit(S[zero]).any(), name
        assert (S[~zero] > 0.0).all(), name
        err = np.abs(S[~zero] - F[~zero]) / F[~zero]
        worst = float(err.max()) if err.size else 0.0
        print("%s T=%d d=%g: largest relative difference %.3g (tol %.3g)" % (name, T, d, worst, tol))
        assert worst <= tol, (name, worst, tol)
        assert np.allclose(F.sum(axis=1), n, rtol=1e-12)          # (the walk keeps its mass: the reference is a walk)
        worst_all = max(worst_all, worst)
    print("recorded maximum error: %.3g" % worst_all)


def test_edge_cases_of_the_recurrence():
    g = ac.degree_graph([0, 1, 4, 5, 9, 0, 2, 0, 30, 3, 0, 7], 5, n_items=60)
    n = len(g["rowptr"]) - 1
    wn, nd = ac.normalise(g)
    S0 = ac.reverse(g, wn, nd, np.arange(n), 0, 0.15)
    assert (S0 == n * np.eye(n)).all()                           # T = 0: n [s = v]
    S = ac.reverse(g, wn, nd, np.arange(n), 6, 0.25)
    dang = np.nonzero(~nd)[0]
    assert len(dang) > 10
    assert (S[dang] == n * np.eye(n)[dang]).all()                # a dangling s: n [s = v] (d = 0.25: rho is exact)
    # d = 0: legal; finite, >= 0
    S = ac.reverse(g, wn, nd, np.arange(n), 5, 0.0)
    assert np.isfinite(S).all() and (S >= 0).all()


def test_rho_host_model_is_numpys_bitwise(tmp_path):
    exe = build_check(tmp_path, sanitize=False)
    for seed, T, d in ((5, 10, float(np.float32(0.15))), (7, 1, 0.5), (8, 4, 1.0), (9, 13, 0.0), (10, 0, 0.3)):
        g = ac.degree_graph([0, 1, 4, 5, 9, 0, 2, 0, 30, 3, 0, 7, 12, 6], seed, n_items=70)
        n = len(g["rowptr"]) - 1
        wn, nd = ac.normalise(g)
        h = ac.dangling_columns(g, wn, nd, T, d)[:T]
        want = ac.rho_table(n, h, T, d) if T else np.zeros((0, n))
        src, out = tmp_path / "h.bin", tmp_path / "rho.bin"
        src.write_bytes(struct.pack("<iiiid", n, T, n, 0, d) + np.ascontiguousarray(h, dtype="<f8").tobytes())
        subprocess.check_call([str(exe), "rho", str(src), str(out)])
        got = np.frombuffer(out.read_bytes(), dtype="<f8").reshape(T, n)
        assert (got.view(np.uint64) == want.view(np.uint64)).all(), (seed, T, d)
