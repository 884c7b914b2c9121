"""Restart-vector walks ranked on the device (rwr_recommend_restart_batch) at the C-ABI and in the host mirrors -- checks that
need no GPU."""
import ctypes as C
import inspect
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "rwr_recommend_restart_batch"


def _lib():
    import __graft_entry__ as ge
    from recommendersystems_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_null_graph_is_refused_first():
    L = _lib()
    lib = L.load()
    ptr = np.array([0, 1, 2], dtype=np.int64)
    idx = np.array([0, 1], dtype=np.int32)
    val = np.array([1.0, 1.0])
    ids, sc, cnt = np.zeros((2, 4), dtype=np.int64), np.zeros((2, 4)), np.zeros(2, dtype=np.int32)
    pp, pi, pv = ptr.ctypes.data_as(C.POINTER(C.c_int64)), idx.ctypes.data_as(C.POINTER(C.c_int32)), \
        val.ctypes.data_as(C.POINTER(C.c_double))
    outs = (ids.ctypes.data_as(C.POINTER(C.c_int64)), sc.ctypes.data_as(C.POINTER(C.c_double)),
            cnt.ctypes.data_as(C.POINTER(C.c_int32)))
    # with a valid batch, with K = 0, with K < 0, with a bad top_n, with nothing else
    for K, top_n, args, o in ((2, 4, (pp, pi, pv, None, pp, pi), outs), (0, 4, (pp, pi, pv, None, None, None), outs),
                              (-1, 4, (pp, pi, pv, None, pp, pi), outs), (2, 0, (pp, pi, pv, None, None, None), outs),
                              (0, 4, (None,) * 6, (None,) * 3)):
        assert getattr(lib, NAME)(None, K, *args, 0.15, 3, top_n, *o) == L.RWR_E_INVALID
        msg = lib.rwr_last_error()
        assert NAME.encode() in msg and b"NULL graph" in msg
    assert not ids.any() and not sc.any() and not cnt.any()


def _params(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S).count(",") + 1


def test_symbol_and_prototypes_agree():
    L = _lib()
    assert NAME in L.EXPORTS
    fn = getattr(L.load(), NAME)
    assert fn is not None and len(fn.argtypes) == 14 and fn.restype is C.c_int32
    assert fn.argtypes[8] is C.c_double and fn.argtypes[9] is C.c_int32 and fn.argtypes[10] is C.c_int32
    hdr = _read("include", "rwr.h")
    m = re.search(r"int32_t\s+%s\s*\(([^;]*)\)\s*;" % NAME, hdr)
    assert m and _params(m.group(1)) == 14
    flat = " ".join(m.group(1).split())
    assert flat == ("rwr_graph *g, int32_t K, const int64_t *sup_ptr, const int32_t *sup_idx, const double *sup_val, "
                    "const int32_t *start, const int64_t *excl_ptr, const int32_t *excl_idx, double d, int32_t n_iter, "
                    "int32_t top_n, int64_t *ids, double *scores, int32_t *counts")
    assert re.search(r'#define\s+RWR_VERSION_STRING\s+"0\.4\.0"', hdr)
    native = _read("csharp", "Recommenders", "RWRBased", "Native.cs")
    m = re.search(r"static extern int %s\(([^)]*)\)" % NAME, native)
    assert m, "Native.cs does not P/Invoke " + NAME
    assert _params(m.group(1)) == 14
    assert " ".join(m.group(1).split()) == ("GraphHandle g, int K, long[] sup_ptr, int[] sup_idx, double[] sup_val, int[] start, "
                                            "long[] excl_ptr, int[] excl_idx, double d, int n_iter, int top_n, long[] ids, "
                                            "double[] scores, int[] counts")
    rec = _read("csharp", "Recommenders", "RWRBased", "Recommender.cs")
    assert re.search(r"public List<KeyValuePair<long, double>>\[\] RecommendationRestartBatch\(int\[\]\[\] nodes, "
                     r"double\[\]\[\] weights, int\[\] start,", rec)
    m = re.search(r"Native\.%s\(([^;]*)\)\);" % NAME, rec)
    assert m and _params(m.group(1)) == 14
    hpp = _read("include", "recommenders", "rwr_based.hpp")
    assert "recommendRestartBatch(" in hpp
    m = re.search(r"check\(%s\(([^;]*)\)\);" % NAME, hpp)
    assert m and _params(m.group(1)) == 14
    assert NAME in _read("INTEGRATION.md")
    assert "RecommendationRestartBatch" in _read("INTEGRATION.md")


def test_python_mirror_signature():
    from recommendersystems_amd.rwr_based import Recommender
    sig = inspect.signature(Recommender.RecommendationRestartBatch)
    assert list(sig.parameters) == ["self", "restarts", "starts", "dampingFactor", "nIteration", "topN", "exclude"]
    assert sig.parameters["exclude"].default is None
