"""CPU-side proof that tests/explain_cases.py's expectation model is the reference's arithmetic, and that every case of
tests/test_gpu_explained.py bites -- from the reference alone, without the library.

The model: a non-seed row's rank after T steps is, bit for bit, the left-to-right sum of its in-entries' addends
fl(fl((1 - d) * x_{T-1}[u]) * w) in in-list order (Model.cs:84-87); checked for every non-seed row and T in {1, 2, 3, 10} on a
weighted and a uniform graph."""
import numpy as np
import pytest

from tests import explain_cases as ec
from tests.test_gpu_typed import bits, oracle_row


@pytest.mark.parametrize("name", ["mixed", "unit", "hub_w", "hub_u"])
def test_addends_sum_to_the_oracles_rank(name):
    g = ec.graph(name)
    n = len(g["node_id"])
    seeds = (2, 9) if name in ("mixed", "unit") else (5,)
    for seed in seeds:
        for T in (1, 2, 3, 10):
            row = oracle_row(g, seed, T)
            for v in range(n):
                if v == seed:
                    continue
                acc = 0.0
                for _, a in ec.addends(g, seed, T, v):
                    acc += a
                assert bits(np.array([acc]))[0] == bits(row[v:v + 1])[0], (name, seed, T, v)
    # the in-lists hold every explicit link once, parallel ones included, and no UNDEFINED one
    explicit = int((g["etype"] != ec.gg.EDGE_UNDEFINED).sum())
    assert sum(len(L) for L in ec.in_lists(g)) == explicit
    for L in ec.in_lists(g):
        assert [u for u, _ in L] == sorted(u for u, _ in L)


def test_the_crafted_graph_has_the_stated_in_degrees():
    for name in ("hub_w", "hub_u"):
        g, items = ec.crafted(name == "hub_u")
        inl = ec.in_lists(ec.graph(name))
        assert [len(inl[v]) for v in items[:-1]] == ec.DEGREES
        assert max(ec.DEGREES) == ec.HUB > 2 * ec.WHY_BLOCK
        pairs = [u for u, _ in inl[items[-1]]]
        assert len(pairs) == 13 and len(set(pairs)) == 12, "two parallel links on one (u, v) pair"
        for r in (1, 2, 8):
            assert {0, 1, r - 1, r, r + 1, 63, 64, 65} <= set(ec.DEGREES)


@pytest.mark.parametrize("case", ec.CASES, ids=lambda c: c["name"])
def test_case_bites(case):
    g = ec.graph(case["graph"])
    r, T, top_n = case["n_why"], case["T"], case["top_n"]
    L = ec.list_rows(g, case)
    assert 0 <= r <= ec.WHY_MAX and len(L) == len(case["seeds"])
    per_entry = [(k, v, ec.addends(g, case["seeds"][k], T, v)) for k, rows in enumerate(L) for v in rows]
    for what in case["bites"]:
        if what == "tie":      # two in-entries with bitwise equal positive addends straddle position n_why of some listed entry
            hit = False
            for _, _, adds in per_entry:
                best = ec.reasons(adds)
                if len(best) > r >= 1 and adds[best[r - 1]][1] == adds[best[r]][1]:
                    hit = True
            assert hit, (case["name"], what)
        elif what == "trunc":
            assert any(len(ec.reasons(adds)) > r for _, _, adds in per_entry), (case["name"], what)
        elif what == "hub":
            assert any(len(ec.in_lists(g)[v]) == ec.HUB and len(ec.reasons(adds)) > 2 * ec.WHY_BLOCK for _, v, adds in per_entry), (case["name"], what)
        elif what == "short":
            assert any(len(rows) < top_n for rows in L), (case["name"], what)
        elif what == "zero":
            assert any(len(ec.reasons(adds)) == 0 for _, _, adds in per_entry), (case["name"], what)
        elif what == "self":   # the seed is listed, and its score is more than its link addends: the restart share is not a reason
            for k, rows in enumerate(L):
                s = case["seeds"][k]
                assert s in rows, (case["name"], what)
                assert sum(a for _, a in ec.addends(g, s, T, s)) < float(oracle_row(g, s, T)[s])
        elif what == "capped":
            free = ec.list_rows(g, dict(case, lab=None))
            assert free != L, (case["name"], "the cap is vacuous")
        elif what == "twins":
            n = len(g["node_id"])
            for rows in L:
                at = rows.index(n - 2)
                assert rows[at + 1] == n - 1, (case["name"], "the twins are adjacent, the smaller row first")
        else:
            raise AssertionError(what)
    if T == 1:                 # the seed is the only reason
        for k, _, adds in per_entry:
            assert all(u == case["seeds"][k] for u, a in adds if a > 0)
    if T == 0:
        assert all(not adds for _, _, adds in per_entry)
