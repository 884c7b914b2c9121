"""Recommendation among the nodes of any node type (rwr_recommend_typed_batch) at the C-ABI and in the host mirrors -- checks
that need no GPU."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "rwr_recommend_typed_batch"


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
    assert fn is not None and len(fn.argtypes) == 12 and fn.restype is C.c_int32
    assert fn.argtypes[3] is C.c_float and fn.argtypes[6] is C.c_int32 and fn.argtypes[7] is C.c_uint32 and fn.argtypes[8] is C.c_int32
    hdr = _read("include", "rwr.h")
    m = re.search(r"int32_t\s+%s\s*\(([^;]*)\)\s*;" % NAME, hdr)
    assert m and _params(m.group(1)) == 12
    assert " ".join(m.group(1).split()) == ("rwr_graph *g, const int32_t *seeds, int32_t K, float d, int32_t n_iter, int32_t top_n, "
                                            "int32_t cand_type, uint32_t excl_edge_mask, int32_t exclude_self, int64_t *ids, "
                                            "double *scores, int32_t *counts")
    assert re.search(r'#define\s+RWR_VERSION_STRING\s+"0\.4\.0"', hdr)
    native = _read("csharp", "Recommenders", "RWRBased", "Native.cs")
    m = re.search(r"static extern int %s\(([^)]*)\)" % NAME, native)
    assert m, "Native.cs does not P/Invoke " + NAME
    assert _params(m.group(1)) == 12
    assert " ".join(m.group(1).split()) == ("GraphHandle g, int[] seeds, int K, float d, int n_iter, int top_n, int cand_type, "
                                            "uint excl_edge_mask, int exclude_self, long[] ids, double[] scores, int[] counts")
    rec = _read("csharp", "Recommenders", "RWRBased", "Recommender.cs")
    assert re.search(r"public List<KeyValuePair<long, double>>\[\] RecommendationTypedBatch\(int\[\] seeds, float dampingFactor, "
                     r"int nIteration, int topN,", rec)
    assert "public List<KeyValuePair<long, double>> RecommendationTyped(int idxTargetNode," in rec
    m = re.search(r"Native\.%s\(([^;]*)\)\);" % NAME, rec)
    assert m and _params(m.group(1)) == 12
    hpp = _read("include", "recommenders", "rwr_based.hpp")
    assert "recommendTypedBatch(" in hpp
    m = re.search(r"check\(%s\(([^;]*)\)\);" % NAME, hpp)
    assert m and _params(m.group(1)) == 12
    assert NAME in _read("INTEGRATION.md") and "RecommendationTypedBatch" in _read("INTEGRATION.md")
    assert "typed.hip" in _read("recommendersystems_amd", "csrc", "Makefile")
    assert "cand_plan.h" in _read("recommendersystems_amd", "csrc", "Makefile")


def test_header_is_c99(tmp_path):
    src = tmp_path / "use_rwr.c"
    src.write_text('#include "rwr.h"\n'
                   "int32_t (*typed)(rwr_graph *, const int32_t *, int32_t, float, int32_t, int32_t, int32_t, uint32_t, int32_t,\n"
                   "                 int64_t *, double *, int32_t *) = rwr_recommend_typed_batch;\n"
                   "int main(void) { return typed == 0; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I",
                           os.path.join(ROOT, "include"), str(src)])


def test_null_graph_is_refused_first():
    L = _lib()
    lib = L.load()
    seeds = np.array([0, 1], dtype=np.int32)
    ids, sc, cnt = np.full((2, 4), -5, dtype=np.int64), np.full((2, 4), -5.0), np.full(2, -5, dtype=np.int32)
    ps = seeds.ctypes.data_as(C.POINTER(C.c_int32))
    outs = (ids.ctypes.data_as(C.POINTER(C.c_int64)), sc.ctypes.data_as(C.POINTER(C.c_double)),
            cnt.ctypes.data_as(C.POINTER(C.c_int32)))
    # with a valid batch, with K = 0, with K < 0, with a bad top_n, candidate type and mask, with nothing else
    for s, K, top_n, cand, mask, o in ((ps, 2, 4, 1, 0x0c, outs), (ps, 0, 4, 1, 0, outs), (ps, -1, 4, 1, 0, outs),
                                       (ps, 2, 0, 999, 0xffff, outs), (None, 0, 4, 1, 0, (None,) * 3)):
        assert getattr(lib, NAME)(None, s, K, C.c_float(0.15), 3, top_n, cand, mask, 1, *o) == L.RWR_E_INVALID
        msg = lib.rwr_last_error()
        assert NAME.encode() in msg and b"NULL graph" in msg
    assert (ids == -5).all() and (sc == -5.0).all() and (cnt == -5).all()


def test_python_mirror_signature():
    from recommendersystems_amd.rwr_based import Recommender
    sig = inspect.signature(Recommender.RecommendationTypedBatch)
    assert list(sig.parameters) == ["self", "seeds", "dampingFactor", "nIteration", "topN", "candType", "exclEdgeTypes",
                                    "excludeSelf"]
    assert sig.parameters["exclEdgeTypes"].default == () and sig.parameters["excludeSelf"].default is False
    sig = inspect.signature(Recommender.RecommendationTyped)
    assert list(sig.parameters) == ["self", "idxTargetNode", "dampingFactor", "nIteration", "topN", "candType", "exclEdgeTypes",
                                    "excludeSelf"]
