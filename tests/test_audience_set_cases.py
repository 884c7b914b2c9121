"""The arithmetic of the audience set entries on the CPU: the reverse recurrence of tests/audience_cases.py started
from g_0 = sum_v a_v e_v against sum_v a_v * (the literal forward loop of Model.cs from s), for EVERY candidate s of the five
small graphs of tests/test_audience_cases.py, sets of 1, 2 and 5 members, weights from {0.25, 1, 3.7}, dangling nodes among and
beside the members -- within the tolerance rwr.h derives, zeros on zeros."""
import numpy as np
import pytest

from tests import audience_cases as ac
from tests.test_audience_cases import _graphs

WEIGHTS = (0.25, 1.0, 3.7)


def reverse_sets(g, wn, nd, sets, weights, T, d):
    """ac.reverse with column k started from sum_v a_v e_v: S[s, k]"""
    n = len(g["rowptr"]) - 1
    rho = ac.rho_table(n, ac.dangling_columns(g, wn, nd, T, d), T, d)
    G = np.zeros((n, len(sets)))
    for k, (mem, a) in enumerate(zip(sets, weights)):
        for v, x in zip(mem, a):
            G[v, k] = G[v, k] + x                                # (members are distinct here; the merge is the plan's)
    S = np.zeros_like(G)
    for j in range(T):
        S = S + rho[T - 1 - j][:, None] * G
        G = ac._back(g, wn, 1 - d, G)
    return S + float(n) * G


def set_tol(g, T, d, m):
    """8 (T + 1) (n + L + m + 8) 2^-53 / d"""
    n = len(g["rowptr"]) - 1
    L = max(int(np.diff(g["rowptr"]).max()), int(np.bincount(g["dst"], minlength=n).max())) if len(g["dst"]) else 0
    return 8.0 * (T + 1) * (n + L + m + 8) * 2.0 ** -53 / d


def _sets(g, nd, seed):
    """sets of 1, 2 and 5 members: one of dangling members only, one mixed, one of non-dangling members where the graph has them"""
    n = len(nd)
    rng = np.random.default_rng(seed)
    dang, live = np.nonzero(~nd)[0], np.nonzero(nd)[0]
    sets = []
    for m in (1, 2, 5):
        m = min(m, n)
        sets.append([int(x) for x in rng.permutation(n)[:m]])
        if len(dang):
            sets.append([int(x) for x in rng.permutation(dang)[:min(m, len(dang))]])
        if len(dang) and len(live) and m > 1:
            sets.append([int(dang[0])] + [int(x) for x in rng.permutation(live)[:m - 1]])
        if len(live):
            sets.append([int(x) for x in rng.permutation(live)[:min(m, len(live))]])
    return sets, [[float(rng.choice(WEIGHTS)) for _ in s] for s in sets]


@pytest.mark.parametrize("T,d", [(0, 0.15), (1, 0.15), (3, 0.5), (4, 1.0), (10, float(np.float32(0.15)))])
def test_reverse_from_a_weighted_set_is_the_weighted_forward_sum(T, d):
    worst_all = 0.0
    for name, g in _graphs():
        n = len(g["rowptr"]) - 1
        wn, nd = ac.normalise(g)
        F = ac.forward(g, wn, nd, np.arange(n), T, d)            # F[s, v]
        sets, weights = _sets(g, nd, 7 + T)
        assert {len(s) for s in sets} >= ({1, 2, 5} if n >= 5 else {1, 2})
        S = reverse_sets(g, wn, nd, sets, weights, T, d)          # S[s, k], every candidate s
        tol = set_tol(g, T, d, max(len(s) for s in sets))
        worst = 0.0
        for k, (mem, a) in enumerate(zip(sets, weights)):
            ref = np.zeros(n)
            for v, x in zip(mem, a):
                ref = ref + x * F[:, v]                          # float64, member order
            zero = ref == 0.0
            assert (S[zero, k] == 0.0).all() and not np.signbit(S[zero, k]).any(), (name, k)
            assert (S[~zero, k] > 0.0).all(), (name, k)
            err = np.abs(S[~zero, k] - ref[~zero]) / ref[~zero]
            worst = max(worst, float(err.max()) if err.size else 0.0)
        print("%s T=%d d=%g: largest relative difference %.3g (tol %.3g)" % (name, T, d, worst, tol))
        assert worst <= tol, (name, worst, tol)
        worst_all = max(worst_all, worst)
    print("recorded maximum error: %.3g" % worst_all)


def test_unit_one_member_sets_are_the_single_target_recurrence_bitwise():
    for name, g in _graphs():
        n = len(g["rowptr"]) - 1
        wn, nd = ac.normalise(g)
        one = ac.reverse(g, wn, nd, np.arange(n), 5, 0.15)
        sets = reverse_sets(g, wn, nd, [[v] for v in range(n)], [[1.0]] * n, 5, 0.15)
        assert (one.view(np.uint64) == sets.view(np.uint64)).all(), name
        scaled = reverse_sets(g, wn, nd, [[v] for v in range(n)], [[2.0 ** -8]] * n, 5, 0.15)
        assert ((one * 2.0 ** -8).view(np.uint64) == scaled.view(np.uint64)).all(), name   # a power of two scales exactly
