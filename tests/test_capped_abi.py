"""Ranked walks with a diversity cap per caller-set group of nodes (rwr_recommend_capped_batch,
rwr_recommend_capped_positions_batch) at the C-ABI and in the host mirrors -- checks that need no GPU."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANKED = "rwr_recommend_capped_batch"
POSITIONS = "rwr_recommend_capped_positions_batch"
HEAD = ("rwr_graph *g, const int32_t *seeds, int32_t K, float d, int32_t n_iter, %sint32_t cand_type, uint32_t excl_edge_mask, "
        "int32_t exclude_self, int64_t pool_count, const int32_t *pool_idx, const int64_t *deny_ptr, const int32_t *deny_idx, "
        "const int32_t *group_of, int32_t group_cap, ")
C_DECL = {RANKED: HEAD % "int32_t top_n, " + "int64_t *ids, double *scores, int32_t *counts",
          POSITIONS: HEAD % "" + "const int64_t *test_ptr, const int64_t *test_ids, int64_t *pos_out, double *score_out, "
                                 "int64_t *list_len"}
CS_HEAD = ("GraphHandle g, int[] seeds, int K, float d, int n_iter, %sint cand_type, uint excl_edge_mask, int exclude_self, "
           "long pool_count, int[] pool_idx, long[] deny_ptr, int[] deny_idx, int[] group_of, int group_cap, ")
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
    sets = [C.c_int32, C.c_uint32, C.c_int32, C.c_int64, p(C.c_int32), p(C.c_int64), p(C.c_int32), p(C.c_int32), C.c_int32]
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
    for method in ("RecommendationCappedBatch(", "RecommendationCapped(", "RecommendationCappedPositionsBatch("):
        assert "public " in rec and method in rec, method
        assert method[:-1] in _read("INTEGRATION.md"), method
    assert "rwr_recommend_capped_batch(" in _read("include", "recommenders", "rwr_based.hpp")
    assert "recommendCappedBatch" in _read("INTEGRATION.md")
    # the limit is the header's, the loader's and the plan's one number
    assert re.search(r"#define\s+RWR_GROUP_CAP_MAX\s+8\b", hdr) and L.RWR_GROUP_CAP_MAX == 8
    assert re.search(r"CAP_MAX\s*=\s*8;", _read("recommendersystems_amd", "csrc", "cap_plan.h"))
    # the contract comment names the consequences and what is out of scope, as the filtered entries name theirs
    doc = hdr[hdr.index("The filtered walks with a diversity cap"):hdr.index("int32_t %s(" % RANKED)]
    for word in ("restart-vector", "Hits / AP", "cap per", "several labellings", "labels kept with the handle", "writes nothing",
                 "do NOT use up", "smaller node index", "RWR_GROUP_CAP_MAX", "group_of == NULL", "RWR_E_UNSUPPORTED", "RWR_E_INVALID"):
        assert word in doc, word
    mk = _read("recommendersystems_amd", "csrc", "Makefile")
    assert "group_cap.hip" in mk and "cap_plan.h" in mk and "group_cap.h " in mk
    assert "3.21" in _read("DESIGN.md") and "RWR_CAP_CHUNK" in _read("DESIGN.md")
    assert "capped_latency.py" in _read("README.md") and os.path.exists(os.path.join(ROOT, "tools", "capped_latency.py"))


def test_header_is_c99(tmp_path):
    src = tmp_path / "use_rwr.c"
    src.write_text('#include "rwr.h"\n'
                   "int32_t (*fr)(rwr_graph *, const int32_t *, int32_t, float, int32_t, int32_t, int32_t, uint32_t, int32_t, int64_t,\n"
                   "              const int32_t *, const int64_t *, const int32_t *, const int32_t *, int32_t, int64_t *, double *,\n"
                   "              int32_t *) = %s;\n"
                   "int32_t (*fp)(rwr_graph *, const int32_t *, int32_t, float, int32_t, int32_t, uint32_t, int32_t, int64_t,\n"
                   "              const int32_t *, const int64_t *, const int32_t *, const int32_t *, int32_t, const int64_t *,\n"
                   "              const int64_t *, int64_t *, double *, int64_t *) = %s;\n"
                   "int cap_max[RWR_GROUP_CAP_MAX == 8 ? 1 : -1];\n"
                   "int main(void) { return fr == 0 || fp == 0 || sizeof cap_max == 0; }\n" % (RANKED, POSITIONS))
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
    lab = np.array([1, 2, 3], dtype=np.int32)
    ids, sc, cnt = np.full((2, 3), -5, dtype=np.int64), np.full((2, 3), -5.0), np.full(2, -5, dtype=np.int32)
    pos, psc, ln = np.full(2, -5, dtype=np.int64), np.full(2, -5.0), np.full(2, -5, dtype=np.int64)
    ps = seeds.ctypes.data_as(PI32)
    flt = (3, pool.ctypes.data_as(PI32), dp.ctypes.data_as(PI64), di.ctypes.data_as(PI32))
    lists = (ids.ctypes.data_as(PI64), sc.ctypes.data_as(PD), cnt.ctypes.data_as(PI32))
    tests = (tp.ctypes.data_as(PI64), ti.ctypes.data_as(PI64), pos.ctypes.data_as(PI64), psc.ctypes.data_as(PD), ln.ctypes.data_as(PI64))
    pl = lab.ctypes.data_as(PI32)
    # with a valid batch, with K = 0, with K < 0, with a bad candidate type, mask, top_n and cap, with nothing else
    for s, K, top_n, cand, mask, f, cap, o, t in ((ps, 2, 3, 1, 0x0c, flt, (pl, 2), lists, tests), (ps, 0, 3, -1, 0, flt, (pl, 0), lists, tests),
                                                  (ps, -1, 3, 1, 0, flt, (None, 0), lists, tests),
                                                  (ps, 2, 1025, 999, 0xffff, flt, (pl, 99), lists, tests),
                                                  (None, 0, 0, -2, 0, (7, None, None, None), (None, -1), (None,) * 3, (None,) * 5)):
        assert lib.rwr_recommend_capped_batch(None, s, K, C.c_float(0.15), 3, top_n, cand, mask, 1, *f, *cap, *o) == L.RWR_E_INVALID
        msg = lib.rwr_last_error()
        assert RANKED.encode() in msg and b"NULL graph" in msg
        assert lib.rwr_recommend_capped_positions_batch(None, s, K, C.c_float(0.15), 3, cand, mask, 1, *f, *cap, *t) == L.RWR_E_INVALID
        msg = lib.rwr_last_error()
        assert POSITIONS.encode() in msg and b"NULL graph" in msg
    assert (ids == -5).all() and (sc == -5.0).all() and (cnt == -5).all()
    assert (pos == -5).all() and (psc == -5.0).all() and (ln == -5).all()


def test_python_mirror_marshals_as_declared(monkeypatch):
    from recommendersystems_amd import _lib as L
    from recommendersystems_amd.rwr_based import Recommender, NodeType, EdgeType
    sig = inspect.signature(Recommender.RecommendationCappedBatch)
    assert list(sig.parameters) == ["self", "seeds", "dampingFactor", "nIteration", "topN", "candType", "exclEdgeTypes", "excludeSelf",
                                    "pool", "deny", "groupOf", "groupCap"]
    assert sig.parameters["candType"].default is None and sig.parameters["exclEdgeTypes"].default == ()
    assert sig.parameters["pool"].default is None and sig.parameters["deny"].default is None
    assert sig.parameters["groupOf"].default is None and sig.parameters["groupCap"].default == 1
    sig = inspect.signature(Recommender.RecommendationCapped)
    assert list(sig.parameters) == ["self", "idxTargetNode", "dampingFactor", "nIteration", "topN", "candType", "exclEdgeTypes",
                                    "excludeSelf", "pool", "deny", "groupOf", "groupCap"]
    sig = inspect.signature(Recommender.RecommendationCappedPositionsBatch)
    assert list(sig.parameters) == ["self", "seeds", "dampingFactor", "nIteration", "testSets", "candType", "exclEdgeTypes",
                                    "excludeSelf", "pool", "deny", "groupOf", "groupCap"]
    seen = {}
    N = 12

    def sets(a, at, K):
        pc = a[at]
        seen.update(pool_count=pc, pool=None if not a[at + 1] else [a[at + 1][q] for q in range(max(pc, 0))])
        if not a[at + 2]:
            seen.update(deny_ptr=None, deny=None)
        else:
            seen["deny_ptr"] = [a[at + 2][k] for k in range(K + 1)]
            seen["deny"] = [a[at + 3][q] for q in range(seen["deny_ptr"][K])]
        seen["group_of"] = None if not a[at + 4] else [a[at + 4][i] for i in range(N)]
        seen["group_ptr"] = None if not a[at + 4] else C.cast(a[at + 4], C.c_void_p).value
        seen["cap"] = a[at + 5]

    class FakeLib:
        @staticmethod
        def rwr_recommend_capped_batch(*a):
            K = a[2]
            seen.update(handle=a[0], seeds=[a[1][k] for k in range(K)], K=K, d=a[3].value, T=a[4], top=a[5], cand=a[6], mask=a[7],
                        self_=a[8])
            sets(a, 9, K)
            for k in range(K):
                a[15][k * a[5]], a[16][k * a[5]], a[17][k] = 70 + k, 0.5 + k, 1
            return 0

        @staticmethod
        def rwr_recommend_capped_positions_batch(*a):
            K = a[2]
            seen.update(handle=a[0], seeds=[a[1][k] for k in range(K)], K=K, d=a[3].value, T=a[4], top=None, cand=a[5], mask=a[6],
                        self_=a[7], ptr=[a[14][k] for k in range(K + 1)])
            sets(a, 8, K)
            seen["ids"] = [a[15][q] for q in range(seen["ptr"][K])]
            for q in range(seen["ptr"][K]):
                a[16][q], a[17][q] = q - 1, 0.25 * q
            for k in range(K):
                a[18][k] = 100 + k
            return 0

    class FakeGraph:
        @staticmethod
        def _handle():
            return 1234

        @staticmethod
        def stats():
            return {"n": N}

    monkeypatch.setattr(L, "load", lambda: FakeLib)
    rec = Recommender.__new__(Recommender)
    rec.graph = FakeGraph
    lab = np.arange(N, dtype=np.int32) % 3 - 1
    ids, sc, cnt = rec.RecommendationCappedBatch([3, 9], 0.25, 7, 4, NodeType.ITEM, (EdgeType.LIKE,), True, pool=[8, 2, 8],
                                                 deny=[[5, 5], ()], groupOf=lab, groupCap=3)
    assert seen["handle"] == 1234 and seen["seeds"] == [3, 9] and seen["K"] == 2 and seen["d"] == 0.25 and seen["T"] == 7
    assert seen["top"] == 4 and seen["cand"] == int(NodeType.ITEM) and seen["self_"] == 1 and seen["mask"] == 1 << int(EdgeType.LIKE)
    assert seen["pool_count"] == 3 and seen["pool"] == [8, 2, 8] and seen["deny_ptr"] == [0, 2, 2] and seen["deny"] == [5, 5]
    assert seen["group_of"] == lab.tolist() and seen["cap"] == 3
    assert seen["group_ptr"] == lab.ctypes.data, "an int32 array is taken as it is"
    assert ids.shape == (2, 4) and ids[:, 0].tolist() == [70, 71] and sc[:, 0].tolist() == [0.5, 1.5] and cnt.tolist() == [1, 1]
    # the defaults: any type, no pool, no deny lists, no labels
    rec.RecommendationCappedBatch([3], 0.25, 7, 4)
    assert seen["cand"] == -1 and seen["mask"] == 0 and seen["self_"] == 0
    assert seen["pool_count"] == -1 and seen["pool"] is None and seen["deny_ptr"] is None and seen["group_of"] is None and seen["cap"] == 1
    # labels of another integer type and as a list are converted; too few labels never reach the library
    rec.RecommendationCappedBatch([3], 0.25, 7, 4, groupOf=lab.astype(np.int64), groupCap=8)
    assert seen["group_of"] == lab.tolist() and seen["cap"] == 8
    rec.RecommendationCappedBatch([3], 0.25, 7, 4, groupOf=lab.tolist(), groupCap=2)
    assert seen["group_of"] == lab.tolist()
    for bad in (lab[:N - 1], []):
        try:
            rec.RecommendationCappedBatch([3], 0.25, 7, 4, groupOf=bad)
        except ValueError as e:
            assert "groupOf" in str(e)
        else:
            raise AssertionError("one label per node is required")
    assert rec.RecommendationCapped(3, 0.25, 7, 4, NodeType.USER, pool=(1, 2), deny=[6], groupOf=lab, groupCap=2) == [(70, 0.5)]
    assert seen["K"] == 1 and seen["cand"] == int(NodeType.USER) and seen["pool"] == [1, 2] and seen["deny_ptr"] == [0, 1]
    assert seen["deny"] == [6] and seen["cap"] == 2
    pos, psc, ln = rec.RecommendationCappedPositionsBatch([3, 9], 0.25, 7, [[11], [12, 12, 13]], None, (EdgeType.FOLLOW,), False,
                                                          pool=np.array([4, 0]), deny=[[1], [2, 3]], groupOf=lab, groupCap=5)
    assert seen["cand"] == -1 and seen["mask"] == 1 << int(EdgeType.FOLLOW) and seen["self_"] == 0 and seen["top"] is None
    assert seen["ptr"] == [0, 1, 4] and seen["ids"] == [11, 12, 12, 13]
    assert seen["pool_count"] == 2 and seen["pool"] == [4, 0] and seen["deny_ptr"] == [0, 1, 3] and seen["deny"] == [1, 2, 3]
    assert seen["group_of"] == lab.tolist() and seen["cap"] == 5 and seen["group_ptr"] == lab.ctypes.data
    assert [p.tolist() for p in pos] == [[-1], [0, 1, 2]] and [s.tolist() for s in psc] == [[0.0], [0.25, 0.5, 0.75]]
    assert ln.tolist() == [100, 101]
