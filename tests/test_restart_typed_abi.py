"""Restart-vector walks ranked among the nodes of any type (rwr_recommend_restart_typed_batch) at the C-ABI and in the host
mirrors -- checks that need no GPU."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "rwr_recommend_restart_typed_batch"


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
    assert NAME in L.EXPORTS
    fn = getattr(L.load(), NAME)
    p = C.POINTER
    assert fn.restype is C.c_int32
    assert fn.argtypes == [C.c_void_p, C.c_int32, p(C.c_int64), p(C.c_int32), p(C.c_double), p(C.c_int32), p(C.c_int64),
                           p(C.c_int32), C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_uint32, C.c_int32, p(C.c_int64),
                           p(C.c_double), p(C.c_int32)]
    hdr = _read("include", "rwr.h")
    m = re.search(r"int32_t\s+%s\s*\(([^;]*)\)\s*;" % NAME, hdr)
    assert m and _params(m.group(1)) == 17
    assert " ".join(m.group(1).split()) == ("rwr_graph *g, int32_t K, const int64_t *sup_ptr, const int32_t *sup_idx, "
                                            "const double *sup_val, const int32_t *start, const int64_t *excl_ptr, "
                                            "const int32_t *excl_idx, double d, int32_t n_iter, int32_t top_n, int32_t cand_type, "
                                            "uint32_t excl_edge_mask, int32_t exclude_members, int64_t *ids, double *scores, "
                                            "int32_t *counts")
    assert re.search(r'#define\s+RWR_VERSION_STRING\s+"0\.4\.0"', hdr)
    native = _read("csharp", "Recommenders", "RWRBased", "Native.cs")
    m = re.search(r"static extern int %s\(([^)]*)\)" % NAME, native)
    assert m, "Native.cs does not P/Invoke " + NAME
    assert " ".join(m.group(1).split()) == ("GraphHandle g, int K, long[] sup_ptr, int[] sup_idx, double[] sup_val, int[] start, "
                                            "long[] excl_ptr, int[] excl_idx, double d, int n_iter, int top_n, int cand_type, "
                                            "uint excl_edge_mask, int exclude_members, long[] ids, double[] scores, int[] counts")
    rec = _read("csharp", "Recommenders", "RWRBased", "Recommender.cs")
    assert re.search(r"public List<KeyValuePair<long, double>>\[\] RecommendationRestartTypedBatch\(int\[\]\[\] nodes, "
                     r"double\[\]\[\] weights, int\[\] start,", rec)
    m = re.search(r"Native\.%s\(([^;]*)\)\);" % NAME, rec)
    assert m and _params(m.group(1)) == 17
    hpp = _read("include", "recommenders", "rwr_based.hpp")
    assert "recommendRestartTypedBatch(" in hpp
    m = re.search(r"check\(%s\(([^;]*)\)\);" % NAME, hpp)
    assert m and _params(m.group(1)) == 17
    assert NAME in _read("INTEGRATION.md") and "RecommendationRestartTypedBatch" in _read("INTEGRATION.md")
    assert NAME in _read("recommendersystems_amd", "csrc", "api.hip")
    assert "3.17" in _read("DESIGN.md") and NAME in _read("DESIGN.md") and NAME in _read("README.md")


def test_header_is_c99(tmp_path):
    src = tmp_path / "use_rwr.c"
    src.write_text('#include "rwr.h"\n'
                   "int32_t (*rt)(rwr_graph *, int32_t, const int64_t *, const int32_t *, const double *, const int32_t *,\n"
                   "              const int64_t *, const int32_t *, double, int32_t, int32_t, int32_t, uint32_t, int32_t,\n"
                   "              int64_t *, double *, int32_t *) = %s;\n"
                   "int main(void) { return rt == 0; }\n" % NAME)
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I",
                           os.path.join(ROOT, "include"), str(src)])


def test_cpp_mirror_compiles(tmp_path):
    src = tmp_path / "use_mirror.cpp"
    src.write_text('#include "recommenders/rwr_based.hpp"\n'
                   "using namespace Recommenders::RWRBased;\n"
                   "std::vector<std::vector<std::pair<int64_t, double>>> f(Recommender &r, const std::vector<std::vector<int>> &ex) {\n"
                   "    return r.recommendRestartTypedBatch({{0, 1}, {2}}, {{1.0, 2.0}, {1.0}}, {}, 0.15, 10, 100, NodeType::USER,\n"
                   "                                        {EdgeType::FRIENDSHIP, EdgeType::FOLLOW}, true, &ex);\n"
                   "}\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                           str(src)])


def test_null_graph_is_refused_first():
    L = _lib()
    lib = L.load()
    ptr = np.array([0, 1, 2], dtype=np.int64)
    idx = np.array([0, 1], dtype=np.int32)
    val = np.array([1.0, 1.0])
    ids, sc, cnt = np.full((2, 4), -5, dtype=np.int64), np.full((2, 4), -5.0), np.full(2, -5, dtype=np.int32)
    pp, pi, pv = ptr.ctypes.data_as(C.POINTER(C.c_int64)), idx.ctypes.data_as(C.POINTER(C.c_int32)), \
        val.ctypes.data_as(C.POINTER(C.c_double))
    outs = (ids.ctypes.data_as(C.POINTER(C.c_int64)), sc.ctypes.data_as(C.POINTER(C.c_double)),
            cnt.ctypes.data_as(C.POINTER(C.c_int32)))
    # with a valid batch, with K = 0, with K < 0, with a bad top_n, candidate type and mask, with nothing else
    for K, top_n, cand, mask, args, o in ((2, 4, 1, 0x0c, (pp, pi, pv, None, pp, pi), outs), (0, 4, 1, 0, (pp, pi, pv, None, None, None), outs),
                                          (-1, 4, 1, 0, (pp, pi, pv, None, pp, pi), outs),
                                          (2, 0, 999, 0xffff, (pp, pi, pv, None, None, None), outs),
                                          (0, 4, 1, 0, (None,) * 6, (None,) * 3)):
        assert getattr(lib, NAME)(None, K, *args, 0.15, 3, top_n, cand, mask, 1, *o) == L.RWR_E_INVALID
        msg = lib.rwr_last_error()
        assert NAME.encode() in msg and b"NULL graph" in msg
    assert (ids == -5).all() and (sc == -5.0).all() and (cnt == -5).all()


def test_python_mirror_marshals_as_declared(monkeypatch):
    from recommendersystems_amd import _lib as L
    from recommendersystems_amd.rwr_based import Recommender, NodeType, EdgeType
    sig = inspect.signature(Recommender.RecommendationRestartTypedBatch)
    assert list(sig.parameters) == ["self", "restarts", "starts", "dampingFactor", "nIteration", "topN", "candType", "exclEdgeTypes",
                                    "excludeMembers", "exclude"]
    assert sig.parameters["exclEdgeTypes"].default == () and sig.parameters["excludeMembers"].default is False
    assert sig.parameters["exclude"].default is None
    seen = {}

    class FakeLib:
        @staticmethod
        def rwr_recommend_restart_typed_batch(*a):
            K = a[1]
            ptr = [a[2][k] for k in range(K + 1)]
            seen.update(handle=a[0], K=K, ptr=ptr, idx=[a[3][q] for q in range(ptr[K])], val=[a[4][q] for q in range(ptr[K])],
                        start=None if a[5] is None else [a[5][k] for k in range(K)],
                        eptr=None if a[6] is None else [a[6][k] for k in range(K + 1)], d=a[8], T=a[9], top=a[10], cand=a[11],
                        mask=a[12], members=a[13])
            seen["eidx"] = None if a[7] is None else [a[7][q] for q in range(seen["eptr"][K])]
            for k in range(K):
                a[14][k * a[10]], a[15][k * a[10]], a[16][k] = 70 + k, 0.25, 1
            return 0

    class FakeGraph:
        n = 50

        @staticmethod
        def _handle():
            return 4321

    monkeypatch.setattr(L, "load", lambda: FakeLib)
    rec = Recommender.__new__(Recommender)
    rec.graph = FakeGraph
    restarts = [{3: 1.0, 5: 2.0}, {7: 0.5}]
    ids, sc, cnt = rec.RecommendationRestartTypedBatch(restarts, [3, -1], 0.15, 10, 4, NodeType.USER,
                                                       (EdgeType.FRIENDSHIP, EdgeType.FOLLOW), True, exclude=[[3, 3], []])
    assert seen["handle"] == 4321 and seen["K"] == 2 and seen["ptr"] == [0, 2, 3]
    assert sorted(zip(seen["idx"][:2], seen["val"][:2])) == [(3, 1.0), (5, 2.0)] and (seen["idx"][2], seen["val"][2]) == (7, 0.5)
    assert seen["start"] == [3, -1] and seen["eptr"] == [0, 2, 2] and seen["eidx"] == [3, 3]
    assert seen["d"] == 0.15 and seen["T"] == 10 and seen["top"] == 4 and seen["cand"] == int(NodeType.USER) and seen["members"] == 1
    assert seen["mask"] == (1 << int(EdgeType.FRIENDSHIP)) | (1 << int(EdgeType.FOLLOW))
    assert ids.shape == (2, 4) and ids[:, 0].tolist() == [70, 71] and sc[0, 0] == 0.25 and cnt.tolist() == [1, 1]
    rec.RecommendationRestartTypedBatch(restarts, [3, -1], 0.15, 10, 4, NodeType.ITEM)
    assert seen["eptr"] is None and seen["eidx"] is None and seen["mask"] == 0 and seen["members"] == 0
