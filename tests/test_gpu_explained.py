"""rwr_recommend_explained_batch on the GPU against tests/explain_cases.py's expectation: ids, scores (bitwise), counts, nodes,
why_src, why_total identical and why_term bitwise equal.  The expectation is the reference's (tests/test_explain_cases.py proves
it on the CPU); the cases are the smallest shapes at which the kernels can go wrong: every in-degree edge of the reasons kernel
(0, 1, n_why - 1 .. n_why + 1, 63 .. 65, a hub of 700 for 256 lanes), n_why in {0, 1, 2, 8}, ties broken by in-list position, T in
{0, 1, 2, 3, 10}, tile widths 1 / 8 / 64 with several tile groups, duplicate and dangling seeds, top_n 1 and 1024, the seed as its
own entry, a pool with deny lists and a cap, and equal (score, id) pairs."""
import numpy as np
import pytest

from tests import explain_cases as ec
from tests.test_gpu_typed import bits, built

pytestmark = pytest.mark.gpu
D = ec.D


@pytest.fixture(scope="module")
def amd():
    import recommendersystems_amd as m
    from recommendersystems_amd import _lib
    assert _lib.load().rwr_device_count() >= 1, "no gfx950 device: the HIP path cannot run"
    return m


def explained(amd, G, case, **kw):
    return amd.Recommender(G).RecommendationExplainedBatch(
        np.asarray(case["seeds"], dtype=np.int32), D, case["T"], case["top_n"], kw.pop("n_why", case["n_why"]), case.get("cand"),
        case.get("edges", ()), case.get("self", False), case.get("pool"), case.get("deny"), case.get("lab"), case.get("m", 1), **kw)


def check(got, want, what):
    names = ("ids", "scores", "counts", "nodes", "why_src", "why_term", "why_total")
    print(what, "counts", got[2].tolist()[:8], "want", want[2].tolist()[:8], "reasons", int(want[6].sum()))
    for name, a, b in zip(names, got, want):
        assert a.shape == b.shape and a.dtype == b.dtype, (what, name, a.shape, b.shape, a.dtype, b.dtype)
        same = (bits(a) == bits(b)) if a.dtype == np.float64 else (a == b)
        bad = np.argwhere(~same)
        assert bad.size == 0, (what, name, "first difference at", bad[0].tolist(), a[tuple(bad[0])], b[tuple(bad[0])], len(bad))


@pytest.mark.parametrize("case", ec.CASES, ids=lambda c: c["name"])
def test_case(amd, case, monkeypatch):
    for k, v in case.get("env", {}).items():
        monkeypatch.setenv(k, v)
    g = ec.graph(case["graph"])
    G = built(amd, g, **case.get("opts", {}))
    check(explained(amd, G, case), ec.expected(g, case), case["name"])


def test_identity_with_the_capped_entry_and_partial_tables(amd):
    case = next(c for c in ec.CASES if c["name"] == "mixed-composed")
    g = ec.graph(case["graph"])
    G = built(amd, g)
    rec = amd.Recommender(G)
    seeds = np.asarray(case["seeds"], dtype=np.int32)
    want = rec.RecommendationCappedBatch(seeds, D, case["T"], case["top_n"], case["cand"], case["edges"], False, case["pool"], case["deny"],
                                         case["lab"], case["m"])
    full = ec.expected(g, case)
    # nothing asked for: the capped call's arrays
    got = explained(amd, G, case, n_why=0, wantNodes=False, wantTotal=False)
    assert got[3] is None and got[6] is None and got[4].shape == (3, case["top_n"], 0)
    for a, b in zip(got[:3], want):
        assert a.tobytes() == b.tobytes()
    # each table alone
    got = explained(amd, G, case, n_why=0, wantTotal=False)
    assert (got[3] == full[3]).all() and got[6] is None
    got = explained(amd, G, case, n_why=0, wantNodes=False)
    assert (got[6] == full[6]).all() and got[3] is None
    got = explained(amd, G, case, wantNodes=False, wantTotal=False)
    assert (got[4] == full[4]).all() and (bits(got[5]) == bits(full[5])).all()
    for a, b in zip(got[:3], want):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", ["hub_u-T3", "twins"])
def test_the_same_call_twice(amd, name):
    case = next(c for c in ec.CASES if c["name"] == name)
    G = built(amd, ec.graph(case["graph"]))
    one, two = explained(amd, G, case), explained(amd, G, case)
    for a, b in zip(one, two):
        assert a.tobytes() == b.tobytes()


def test_one_seed_mirror(amd):
    case = next(c for c in ec.CASES if c["name"] == "hub_w-r2")
    g = ec.graph(case["graph"])
    want = ec.expected(g, dict(case, seeds=case["seeds"][:1]))
    lst, nodes, src, term, total = amd.Recommender(built(amd, g)).RecommendationExplained(case["seeds"][0], D, case["T"], case["top_n"], 2,
                                                                                         case["cand"])
    c = int(want[2][0])
    assert [x[0] for x in lst] == want[0][0, :c].tolist() and nodes.tolist() == want[3][0, :c].tolist()
    assert src.tolist() == want[4][0, :c].tolist() and (bits(term) == bits(want[5][0, :c])).all() and total.tolist() == want[6][0, :c].tolist()


def test_refusals_in_their_order_write_nothing(amd):
    import ctypes as C
    from recommendersystems_amd import _lib as L
    lib = L.load()
    g = ec.graph("mixed")
    G = built(amd, g)
    n = len(g["node_id"])
    PI32, PI64, PD = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)
    seeds = np.array([0, 1], dtype=np.int32)
    lab = np.zeros(n, dtype=np.int32)
    ids, sc, cnt = np.full((2, 2000), -5, dtype=np.int64), np.full((2, 2000), -5.0), np.full(2, -5, dtype=np.int32)
    nodes, src = np.full((2, 2000), -5, dtype=np.int32), np.full((2, 2000, 9), -5, dtype=np.int32)
    term, total = np.full((2, 2000, 9), -5.0), np.full((2, 2000), -5, dtype=np.int64)

    def call(top_n, cap, r, with_src=True, d=0.15):
        return lib.rwr_recommend_explained_batch(G._handle(), seeds.ctypes.data_as(PI32), 2, C.c_float(d), 3, top_n, 2, 0, 0, -1, None, None,
                                                 None, lab.ctypes.data_as(PI32), cap, r, ids.ctypes.data_as(PI64), sc.ctypes.data_as(PD),
                                                 cnt.ctypes.data_as(PI32), nodes.ctypes.data_as(PI32),
                                                 src.ctypes.data_as(PI32) if with_src else None, term.ctypes.data_as(PD),
                                                 total.ctypes.data_as(PI64))

    # every later fault is present in every call: the documented order peels them off one by one
    for args, status, word in (((2000, 0, -1, False, 7.0), L.RWR_E_INVALID, b"group_cap"),
                               ((2000, 99, -1, False, 7.0), L.RWR_E_INVALID, b"n_why"),
                               ((2000, 99, 99, False, 7.0), L.RWR_E_INVALID, b"why_src"),
                               ((2000, 99, 99, True, 7.0), L.RWR_E_UNSUPPORTED, b"1024"),
                               ((10, 99, 99, True, 7.0), L.RWR_E_UNSUPPORTED, b"RWR_GROUP_CAP_MAX = 8"),
                               ((10, 8, 99, True, 7.0), L.RWR_E_UNSUPPORTED, b"RWR_WHY_MAX = 8"),
                               ((10, 8, 8, True, 7.0), L.RWR_E_UNSUPPORTED, b"damping")):
        assert call(*args) == status, (args, lib.rwr_last_error())
        msg = lib.rwr_last_error()
        assert b"rwr_recommend_explained_batch" in msg and word in msg, (args, msg)
    for a in (ids, sc, cnt, nodes, src, term, total):
        assert (a == -5).all()
    assert call(10, 8, 8) == L.RWR_OK, lib.rwr_last_error()
