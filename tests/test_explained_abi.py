"""The reasons of ranked entries (rwr_recommend_explained_batch) at the C-ABI and in the host mirrors -- checks that need no GPU.
The argument verdicts beyond the NULL graph are typed_call.h's, checked in their order by tests/test_typed_call.py; here the
header's text states that order."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "rwr_recommend_explained_batch"
C_DECL = ("rwr_graph *g, const int32_t *seeds, int32_t K, float d, int32_t n_iter, int32_t top_n, int32_t cand_type, "
          "uint32_t excl_edge_mask, int32_t exclude_self, int64_t pool_count, const int32_t *pool_idx, const int64_t *deny_ptr, "
          "const int32_t *deny_idx, const int32_t *group_of, int32_t group_cap, int32_t n_why, int64_t *ids, double *scores, "
          "int32_t *counts, int32_t *nodes, int32_t *why_src, double *why_term, int64_t *why_total")
CS_DECL = ("GraphHandle g, int[] seeds, int K, float d, int n_iter, int top_n, int cand_type, uint excl_edge_mask, int exclude_self, "
           "long pool_count, int[] pool_idx, long[] deny_ptr, int[] deny_idx, int[] group_of, int group_cap, int n_why, long[] ids, "
           "double[] scores, int[] counts, int[] nodes, int[] why_src, double[] why_term, long[] why_total")


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


def test_symbol_and_prototypes_agree():
    L = _lib()
    lib = L.load()
    p = C.POINTER
    want = [C.c_void_p, p(C.c_int32), C.c_int32, C.c_float, C.c_int32, C.c_int32, C.c_int32, C.c_uint32, C.c_int32, C.c_int64,
            p(C.c_int32), p(C.c_int64), p(C.c_int32), p(C.c_int32), C.c_int32, C.c_int32, p(C.c_int64), p(C.c_double), p(C.c_int32),
            p(C.c_int32), p(C.c_int32), p(C.c_double), p(C.c_int64)]
    hdr = _read("include", "rwr.h")
    native = _read("csharp", "Recommenders", "RWRBased", "Native.cs")
    rec = _read("csharp", "Recommenders", "RWRBased", "Recommender.cs")
    assert NAME in L.EXPORTS
    fn = getattr(lib, NAME)
    assert fn.restype is C.c_int32 and fn.argtypes == want
    m = re.search(r"int32_t\s+%s\s*\(([^;]*)\)\s*;" % NAME, hdr)
    assert m and _params(m.group(1)) == len(want) == 23
    assert " ".join(re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split()).replace(" ,", ",") == C_DECL
    m = re.search(r"static extern int %s\(([^)]*)\)" % NAME, native)
    assert m, "Native.cs does not P/Invoke " + NAME
    assert " ".join(m.group(1).split()) == CS_DECL
    m = re.search(r"Native\.%s\(([^;]*)\)\);" % NAME, rec)
    assert m and _params(m.group(1)) == len(want)
    for doc in ("INTEGRATION.md", "DESIGN.md", "README.md"):
        assert NAME in _read(doc), doc
    assert NAME in _read("recommendersystems_amd", "csrc", "api.hip")
    for method in ("RecommendationExplainedBatch(", "RecommendationExplained("):
        assert "public " in rec and method in rec, method
        assert method[:-1] in _read("INTEGRATION.md"), method
    assert NAME + "(" in _read("include", "recommenders", "rwr_based.hpp")
    assert "recommendExplainedBatch" in _read("INTEGRATION.md")
    # the limit is the header's, the loader's and the plan's one number; the version stays
    assert re.search(r"#define\s+RWR_WHY_MAX\s+8\b", hdr) and L.RWR_WHY_MAX == 8
    assert re.search(r"WHY_MAX\s*=\s*8;", _read("recommendersystems_amd", "csrc", "explain_plan.h"))
    assert '"0.4.0"' in hdr
    # the contract comment: the definitions, the order of the refusals, and what is out of scope
    doc = " ".join(hdr[hdr.index('"Why is this entry here?"'):hdr.index("int32_t %s(" % NAME)].replace("\n *", " ").split())
    for word in ("bitwise those of the capped entry", "smaller node index", "hold -1", "source ascending", "Parallel links",
                 "UNDEFINED links are not entries", "fl(fl(c1 * y[u_e]) * w_e)", "no FMA", "a_e > 0", "a_e descending",
                 "in-list position ascending", "-1 / +0.0", "why_total", "T <= 0", "restart share", "is not listed", "RWR_WHY_MAX",
                 "launch for launch", "writes nothing", "RWR_E_INVALID", "RWR_E_UNSUPPORTED", "restart-vector", "two-hop",
                 "edge type of a reason", "evaluating and the positions"):
        assert word in doc, word
    order = [doc.index(w) for w in ("up to and including group_cap < 1", "n_why < 0", "the limits", "n_why > RWR_WHY_MAX", "; the domain.")]
    assert order == sorted(order)
    mk = _read("recommendersystems_amd", "csrc", "Makefile")
    assert "explain.hip" in mk and "explain_plan.h" in mk and "explain.h " in mk
    assert "3.22" in _read("DESIGN.md")
    assert "explained_latency.py" in _read("README.md") and os.path.exists(os.path.join(ROOT, "tools", "explained_latency.py"))
    assert "explained_C2.jsonl" in _read("profiles", "README.md")


def test_header_is_c99(tmp_path):
    src = tmp_path / "use_rwr.c"
    src.write_text('#include "rwr.h"\n'
                   "int32_t (*fe)(rwr_graph *, const int32_t *, int32_t, float, int32_t, int32_t, int32_t, uint32_t, int32_t, int64_t,\n"
                   "              const int32_t *, const int64_t *, const int32_t *, const int32_t *, int32_t, int32_t, int64_t *, double *,\n"
                   "              int32_t *, int32_t *, int32_t *, double *, int64_t *) = %s;\n"
                   "int why_max[RWR_WHY_MAX == 8 ? 1 : -1];\n"
                   "int main(void) { return fe == 0 || sizeof why_max == 0; }\n" % NAME)
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I",
                           os.path.join(ROOT, "include"), str(src)])


def test_null_graph_is_refused_first():
    L = _lib()
    lib = L.load()
    PI32, PI64, PD = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)
    seeds = np.array([0, 1], dtype=np.int32)
    pool = np.array([5, 5, -3], dtype=np.int32)
    dp, di = np.array([0, 1, 2], dtype=np.int64), np.array([0, 99], dtype=np.int32)
    lab = np.array([1, 2, 3], dtype=np.int32)
    ids, sc, cnt = np.full((2, 3), -5, dtype=np.int64), np.full((2, 3), -5.0), np.full(2, -5, dtype=np.int32)
    nodes, src, term = np.full((2, 3), -5, dtype=np.int32), np.full((2, 3, 8), -5, dtype=np.int32), np.full((2, 3, 8), -5.0)
    total = np.full((2, 3), -5, dtype=np.int64)
    ps = seeds.ctypes.data_as(PI32)
    flt = (3, pool.ctypes.data_as(PI32), dp.ctypes.data_as(PI64), di.ctypes.data_as(PI32))
    lists = (ids.ctypes.data_as(PI64), sc.ctypes.data_as(PD), cnt.ctypes.data_as(PI32))
    why = (nodes.ctypes.data_as(PI32), src.ctypes.data_as(PI32), term.ctypes.data_as(PD), total.ctypes.data_as(PI64))
    pl = lab.ctypes.data_as(PI32)
    # with a valid batch, with K = 0, with K < 0, with every later fault present, with nothing else
    for s, K, top_n, cand, mask, f, cap, r, o, w in ((ps, 2, 3, 1, 0x0c, flt, (pl, 2), 3, lists, why), (ps, 0, 3, -1, 0, flt, (pl, 0), 0, lists, why),
                                                     (ps, -1, 3, 1, 0, flt, (None, 0), 8, lists, why),
                                                     (ps, 2, 1025, 999, 0xffff, flt, (pl, 99), 99, lists, (None,) * 4),
                                                     (None, 0, 0, -2, 0, (7, None, None, None), (None, -1), -1, (None,) * 3, (None,) * 4)):
        assert lib.rwr_recommend_explained_batch(None, s, K, C.c_float(0.15), 3, top_n, cand, mask, 1, *f, *cap, r, *o, *w) == L.RWR_E_INVALID
        msg = lib.rwr_last_error()
        assert NAME.encode() in msg and b"NULL graph" in msg
    for a in (ids, sc, cnt, nodes, src, term, total):
        assert (a == -5).all()


def test_python_mirror_marshals_as_declared(monkeypatch):
    from recommendersystems_amd import _lib as L
    from recommendersystems_amd.rwr_based import Recommender, NodeType, EdgeType
    sig = inspect.signature(Recommender.RecommendationExplainedBatch)
    assert list(sig.parameters) == ["self", "seeds", "dampingFactor", "nIteration", "topN", "nWhy", "candType", "exclEdgeTypes",
                                    "excludeSelf", "pool", "deny", "groupOf", "groupCap", "wantNodes", "wantTotal"]
    assert sig.parameters["nWhy"].default == 3 and sig.parameters["groupOf"].default is None
    assert sig.parameters["wantNodes"].default is True and sig.parameters["wantTotal"].default is True
    sig = inspect.signature(Recommender.RecommendationExplained)
    assert list(sig.parameters) == ["self", "idxTargetNode", "dampingFactor", "nIteration", "topN", "nWhy", "candType", "exclEdgeTypes",
                                    "excludeSelf", "pool", "deny", "groupOf", "groupCap"]
    seen = {}
    N = 12

    class FakeLib:
        @staticmethod
        def rwr_recommend_explained_batch(*a):
            K, top, r = a[2], a[5], a[15]
            seen.update(handle=a[0], seeds=[a[1][k] for k in range(K)], K=K, d=a[3].value, T=a[4], top=top, cand=a[6], mask=a[7], self_=a[8],
                        pool_count=a[9], pool=None if not a[10] else [a[10][q] for q in range(max(a[9], 0))],
                        deny_ptr=None if not a[11] else [a[11][k] for k in range(K + 1)],
                        group_of=None if not a[13] else [a[13][i] for i in range(N)], cap=a[14], r=r, nodes=bool(a[19]), total=bool(a[22]))
            for k in range(K):
                a[16][k * top], a[17][k * top], a[18][k] = 70 + k, 0.5 + k, 1
                if a[19]:
                    a[19][k * top] = 40 + k
                if a[22]:
                    a[22][k * top] = 9
                for i in range(r):
                    a[20][k * top * r + i], a[21][k * top * r + i] = 100 * k + i, 0.25 * (i + 1)
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
    ids, sc, cnt, nodes, src, term, total = rec.RecommendationExplainedBatch([3, 9], 0.25, 7, 4, 2, NodeType.ITEM, (EdgeType.LIKE,), True,
                                                                             pool=[8, 2, 8], deny=[[5, 5], ()], groupOf=lab, groupCap=3)
    assert seen["handle"] == 1234 and seen["seeds"] == [3, 9] and seen["d"] == 0.25 and seen["T"] == 7 and seen["top"] == 4
    assert seen["cand"] == int(NodeType.ITEM) and seen["self_"] == 1 and seen["mask"] == 1 << int(EdgeType.LIKE) and seen["r"] == 2
    assert seen["pool_count"] == 3 and seen["pool"] == [8, 2, 8] and seen["deny_ptr"] == [0, 2, 2]
    assert seen["group_of"] == lab.tolist() and seen["cap"] == 3 and seen["nodes"] and seen["total"]
    assert ids.shape == (2, 4) and ids[:, 0].tolist() == [70, 71] and cnt.tolist() == [1, 1]
    assert nodes.shape == (2, 4) and nodes.dtype == np.int32 and nodes[:, 0].tolist() == [40, 41] and nodes[0, 1] == -1
    assert src.shape == (2, 4, 2) and src.dtype == np.int32 and src[1, 0].tolist() == [100, 101] and src[0, 1].tolist() == [-1, -1]
    assert term.shape == (2, 4, 2) and term[0, 0].tolist() == [0.25, 0.5] and total.dtype == np.int64 and total[:, 0].tolist() == [9, 9]
    # the defaults; tables that are not wanted are NULL and come back as None
    out = rec.RecommendationExplainedBatch([3], 0.25, 7, 4, 0, wantNodes=False, wantTotal=False)
    assert seen["cand"] == -1 and seen["mask"] == 0 and seen["pool_count"] == -1 and seen["deny_ptr"] is None and seen["group_of"] is None
    assert seen["r"] == 0 and not seen["nodes"] and not seen["total"] and out[3] is None and out[6] is None and out[4].shape == (1, 4, 0)
    lst, nodes, src, term, total = rec.RecommendationExplained(3, 0.25, 7, 4, 1, NodeType.USER, deny=[6])
    assert lst == [(70, 0.5)] and nodes.tolist() == [40] and src.tolist() == [[0]] and term.tolist() == [[0.25]] and total.tolist() == [9]
    assert seen["K"] == 1 and seen["deny_ptr"] == [0, 1]
