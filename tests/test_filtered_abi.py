"""Ranked walks within a caller-set pool and with per-seed deny lists (rwr_recommend_filtered_batch,
rwr_recommend_filtered_positions_batch) at the C-ABI and in the host mirrors -- checks that need no GPU."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANKED = "rwr_recommend_filtered_batch"
POSITIONS = "rwr_recommend_filtered_positions_batch"
HEAD = ("rwr_graph *g, const int32_t *seeds, int32_t K, float d, int32_t n_iter, %sint32_t cand_type, uint32_t excl_edge_mask, "
        "int32_t exclude_self, int64_t pool_count, const int32_t *pool_idx, const int64_t *deny_ptr, const int32_t *deny_idx, ")
C_DECL = {RANKED: HEAD % "int32_t top_n, " + "int64_t *ids, double *scores, int32_t *counts",
          POSITIONS: HEAD % "" + "const int64_t *test_ptr, const int64_t *test_ids, int64_t *pos_out, double *score_out, "
                                 "int64_t *list_len"}
CS_HEAD = ("GraphHandle g, int[] seeds, int K, float d, int n_iter, %sint cand_type, uint excl_edge_mask, int exclude_self, "
           "long pool_count, int[] pool_idx, long[] deny_ptr, int[] deny_idx, ")
CS_DECL = {RANKED: CS_HEAD % "int top_n, " + "long[] ids, double[] scores, int[] counts",
           POSITIONS: CS_HEAD % "" + "long[] test_ptr, long[] test_ids, long[] pos_out, double[] score_out, long[] list_len"}


def _lib():
    import __graft_entry__ as ge
    from recommendersystems_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def _params(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S).count(",") + 1


def test_symbols_and_prototypes_agree():
    L = _lib()
    lib = L.load()
    p = C.POINTER
    head = [C.c_void_p, p(C.c_int32), C.c_int32, C.c_float, C.c_int32]
    sets = [C.c_int32, C.c_uint32, C.c_int32, C.c_int64, p(C.c_int32), p(C.c_int64), p(C.c_int32)]
    want = {RANKED: head + [C.c_int32] + sets + [p(C.c_int64), p(C.c_double), p(C.c_int32)],
            POSITIONS: head + sets + [p(C.c_int64), p(C.c_int64), p(C.c_int64), p(C.c_double), p(C.c_int64)]}
    hdr = _read("include", "rwr.h")
    native = _read("csharp", "Recommenders", "RWRBased", "Native.cs")
    rec = _read("csharp", "Recommenders", "RWRBased", "Recommender.cs")
    for name in (RANKED, POSITIONS):
        assert name in L.EXPORTS
        fn = getattr(lib, name)
        assert fn.restype is C.c_int32 and fn.argtypes == want[name], name
        m = re.search(r"int32_t\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert m and _params(m.group(1)) == len(want[name])
        assert " ".join(re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split()).replace(" ,", ",") == C_DECL[name]
        m = re.search(r"static extern int %s\(([^)]*)\)" % name, native)
        assert m, "Native.cs does not P/Invoke " + name
        assert " ".join(m.group(1).split()) == CS_DECL[name]
        m = re.search(r"Native\.%s\(([^;]*)\)\);" % name, rec)
        assert m and _params(m.group(1)) == len(want[name])
        assert name in _read("INTEGRATION.md") and name in _read("recommendersystems_amd", "csrc", "api.hip")
        assert name in _read("DESIGN.md") and name in _read("README.md")
    for method in ("RecommendationFilteredBatch(", "RecommendationFiltered(", "RecommendationFilteredPositionsBatch("):
        assert "public " in rec and method in rec, method
        assert method[:-1] in _read("INTEGRATION.md"), method
    # the contract comment names what is out of scope, as the typed entries name theirs
    doc = hdr[hdr.index("The typed walks ranked within a candidate pool"):hdr.index("int32_t %s(" % RANKED)]
    for word in ("restart-vector", "pool per", "node ids instead of indices", "RWR_E_RANGE", "writes nothing", "[-1, 255]"):
        assert word in doc, word
    mk = _read("recommendersystems_amd", "csrc", "Makefile")
    assert "filter.hip" in mk and "filter_plan.h" in mk and "filter.h " in mk
    assert "3.20" in _read("DESIGN.md")


def test_header_is_c99(tmp_path):
    src = tmp_path / "use_rwr.c"
    src.write_text('#include "rwr.h"\n'
                   "int32_t (*fr)(rwr_graph *, const int32_t *, int32_t, float, int32_t, int32_t, int32_t, uint32_t, int32_t, int64_t,\n"
                   "              const int32_t *, const int64_t *, const int32_t *, int64_t *, double *, int32_t *) = %s;\n"
                   "int32_t (*fp)(rwr_graph *, const int32_t *, int32_t, float, int32_t, int32_t, uint32_t, int32_t, int64_t,\n"
                   "              const int32_t *, const int64_t *, const int32_t *, const int64_t *, const int64_t *, int64_t *,\n"
                   "              double *, int64_t *) = %s;\n"
                   "int main(void) { return fr == 0 || fp == 0; }\n" % (RANKED, POSITIONS))
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I",
                           os.path.join(ROOT, "include"), str(src)])


def test_null_graph_is_refused_first():
    L = _lib()
    lib = L.load()
    PI32, PI64, PD = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)
    seeds = np.array([0, 1], dtype=np.int32)
    pool = np.array([5, 5, -3], dtype=np.int32)
    dp, di = np.array([0, 1, 2], dtype=np.int64), np.array([0, 99], dtype=np.int32)
    tp, ti = np.array([0, 1, 2], dtype=np.int64), np.array([4, 5], dtype=np.int64)
    ids, sc, cnt = np.full((2, 3), -5, dtype=np.int64), np.full((2, 3), -5.0), np.full(2, -5, dtype=np.int32)
    pos, psc, ln = np.full(2, -5, dtype=np.int64), np.full(2, -5.0), np.full(2, -5, dtype=np.int64)
    ps = seeds.ctypes.data_as(PI32)
    flt = (3, pool.ctypes.data_as(PI32), dp.ctypes.data_as(PI64), di.ctypes.data_as(PI32))
    lists = (ids.ctypes.data_as(PI64), sc.ctypes.data_as(PD), cnt.ctypes.data_as(PI32))
    tests = (tp.ctypes.data_as(PI64), ti.ctypes.data_as(PI64), pos.ctypes.data_as(PI64), psc.ctypes.data_as(PD), ln.ctypes.data_as(PI64))
    # with a valid batch, with K = 0, with K < 0, with a bad candidate type, mask and top_n, with nothing else
    for s, K, top_n, cand, mask, f, o, t in ((ps, 2, 3, 1, 0x0c, flt, lists, tests), (ps, 0, 3, -1, 0, flt, lists, tests),
                                             (ps, -1, 3, 1, 0, flt, lists, tests), (ps, 2, 1025, 999, 0xffff, flt, lists, tests),
                                             (None, 0, 0, -2, 0, (7, None, None, None), (None,) * 3, (None,) * 5)):
        assert lib.rwr_recommend_filtered_batch(None, s, K, C.c_float(0.15), 3, top_n, cand, mask, 1, *f, *o) == L.RWR_E_INVALID
        msg = lib.rwr_last_error()
        assert RANKED.encode() in msg and b"NULL graph" in msg
        assert lib.rwr_recommend_filtered_positions_batch(None, s, K, C.c_float(0.15), 3, cand, mask, 1, *f, *t) == L.RWR_E_INVALID
        msg = lib.rwr_last_error()
        assert POSITIONS.encode() in msg and b"NULL graph" in msg
    assert (ids == -5).all() and (sc == -5.0).all() and (cnt == -5).all()
    assert (pos == -5).all() and (psc == -5.0).all() and (ln == -5).all()


def test_python_mirror_marshals_as_declared(monkeypatch):
    from recommendersystems_amd import _lib as L
    from recommendersystems_amd.rwr_based import Recommender, NodeType, EdgeType
    sig = inspect.signature(Recommender.RecommendationFilteredBatch)
    assert list(sig.parameters) == ["self", "seeds", "dampingFactor", "nIteration", "topN", "candType", "exclEdgeTypes", "excludeSelf",
                                    "pool", "deny"]
    assert sig.parameters["candType"].default is None and sig.parameters["exclEdgeTypes"].default == ()
    assert sig.parameters["excludeSelf"].default is False and sig.parameters["pool"].default is None
    assert sig.parameters["deny"].default is None
    sig = inspect.signature(Recommender.RecommendationFiltered)
    assert list(sig.parameters) == ["self", "idxTargetNode", "dampingFactor", "nIteration", "topN", "candType", "exclEdgeTypes",
                                    "excludeSelf", "pool", "deny"]
    sig = inspect.signature(Recommender.RecommendationFilteredPositionsBatch)
    assert list(sig.parameters) == ["self", "seeds", "dampingFactor", "nIteration", "testSets", "candType", "exclEdgeTypes",
                                    "excludeSelf", "pool", "deny"]
    seen = {}

    def sets(a, at, K):
        pc = a[at]
        seen.update(pool_count=pc, pool=None if not a[at + 1] else [a[at + 1][q] for q in range(max(pc, 0))])
        if not a[at + 2]:
            seen.update(deny_ptr=None, deny=None)
        else:
            seen["deny_ptr"] = [a[at + 2][k] for k in range(K + 1)]
            seen["deny"] = [a[at + 3][q] for q in range(seen["deny_ptr"][K])]

    class FakeLib:
        @staticmethod
        def rwr_recommend_filtered_batch(*a):
            K = a[2]
            seen.update(handle=a[0], seeds=[a[1][k] for k in range(K)], K=K, d=a[3].value, T=a[4], top=a[5], cand=a[6], mask=a[7],
                        self_=a[8])
            sets(a, 9, K)
            for k in range(K):
                a[13][k * a[5]], a[14][k * a[5]], a[15][k] = 70 + k, 0.5 + k, 1
            return 0

        @staticmethod
        def rwr_recommend_filtered_positions_batch(*a):
            K = a[2]
            seen.update(handle=a[0], seeds=[a[1][k] for k in range(K)], K=K, d=a[3].value, T=a[4], top=None, cand=a[5], mask=a[6],
                        self_=a[7], ptr=[a[12][k] for k in range(K + 1)])
            sets(a, 8, K)
            seen["ids"] = [a[13][q] for q in range(seen["ptr"][K])]
            for q in range(seen["ptr"][K]):
                a[14][q], a[15][q] = q - 1, 0.25 * q
            for k in range(K):
                a[16][k] = 100 + k
            return 0

    class FakeGraph:
        @staticmethod
        def _handle():
            return 1234

    monkeypatch.setattr(L, "load", lambda: FakeLib)
    rec = Recommender.__new__(Recommender)
    rec.graph = FakeGraph
    ids, sc, cnt = rec.RecommendationFilteredBatch([3, 9], 0.25, 7, 4, NodeType.ITEM, (EdgeType.LIKE,), True, pool=[8, 2, 8],
                                                   deny=[[5, 5], ()])
    assert seen["handle"] == 1234 and seen["seeds"] == [3, 9] and seen["K"] == 2 and seen["d"] == 0.25 and seen["T"] == 7
    assert seen["top"] == 4 and seen["cand"] == int(NodeType.ITEM) and seen["self_"] == 1 and seen["mask"] == 1 << int(EdgeType.LIKE)
    assert seen["pool_count"] == 3 and seen["pool"] == [8, 2, 8] and seen["deny_ptr"] == [0, 2, 2] and seen["deny"] == [5, 5]
    assert ids.shape == (2, 4) and ids[:, 0].tolist() == [70, 71] and sc[:, 0].tolist() == [0.5, 1.5] and cnt.tolist() == [1, 1]
    # the defaults: any type, no pool, no deny lists; an empty pool is count 0 behind a valid pointer
    rec.RecommendationFilteredBatch([3], 0.25, 7, 4)
    assert seen["cand"] == -1 and seen["mask"] == 0 and seen["self_"] == 0
    assert seen["pool_count"] == -1 and seen["pool"] is None and seen["deny_ptr"] is None
    rec.RecommendationFilteredBatch([3], 0.25, 7, 4, pool=[], deny=[[]])
    assert seen["pool_count"] == 0 and seen["pool"] == [] and seen["deny_ptr"] == [0, 0] and seen["deny"] == []
    assert rec.RecommendationFiltered(3, 0.25, 7, 4, NodeType.USER, pool=(1, 2), deny=[6]) == [(70, 0.5)]
    assert seen["K"] == 1 and seen["cand"] == int(NodeType.USER) and seen["pool"] == [1, 2] and seen["deny_ptr"] == [0, 1]
    assert seen["deny"] == [6]
    pos, psc, ln = rec.RecommendationFilteredPositionsBatch([3, 9], 0.25, 7, [[11], [12, 12, 13]], None, (EdgeType.FOLLOW,), False,
                                                            pool=np.array([4, 0]), deny=[[1], [2, 3]])
    assert seen["cand"] == -1 and seen["mask"] == 1 << int(EdgeType.FOLLOW) and seen["self_"] == 0 and seen["top"] is None
    assert seen["ptr"] == [0, 1, 4] and seen["ids"] == [11, 12, 12, 13]
    assert seen["pool_count"] == 2 and seen["pool"] == [4, 0] and seen["deny_ptr"] == [0, 1, 3] and seen["deny"] == [1, 2, 3]
    assert [p.tolist() for p in pos] == [[-1], [0, 1, 2]] and [s.tolist() for s in psc] == [[0.0], [0.25, 0.5, 0.75]]
    assert ln.tolist() == [100, 101]
    try:
        rec.RecommendationFilteredBatch([3, 9], 0.25, 7, 4, deny=[[1]])
    except ValueError as e:
        assert "deny" in str(e)
    else:
        raise AssertionError("a deny list per seed is required")
