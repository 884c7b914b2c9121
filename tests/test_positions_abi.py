"""Positions and scores of held-out ids in whole typed lists (rwr_recommend_typed_positions_batch,
rwr_recommend_restart_typed_positions_batch) at the C-ABI and in the host mirrors -- checks that need no GPU.  The refusals
with a real graph behind them are in tests/test_gpu_positions.py; here a block of zeros stands in for the handle (a graph of no
nodes whose weights were never found non-negative), which is all the argument checks read of it."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPED = "rwr_recommend_typed_positions_batch"
RESTART = "rwr_recommend_restart_typed_positions_batch"
P64, P32, PD = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_double)


def _lib():
    import __graft_entry__ as ge
    from recommendersystems_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def _flat(text):
    return " ".join(re.sub(r"/\*.*?\*/", "", text, flags=re.S).split()).replace(" ,", ",")


def test_symbols_and_prototypes_agree():
    L = _lib()
    lib = L.load()
    p = C.POINTER
    hdr = _read("include", "rwr.h")
    native = _read("csharp", "Recommenders", "RWRBased", "Native.cs")
    rec = _read("csharp", "Recommenders", "RWRBased", "Recommender.cs")
    want = {
        TYPED: ([C.c_void_p, p(C.c_int32), C.c_int32, C.c_float, C.c_int32, C.c_int32, C.c_uint32, C.c_int32, p(C.c_int64),
                 p(C.c_int64), p(C.c_int64), p(C.c_double), p(C.c_int64)],
                "rwr_graph *g, const int32_t *seeds, int32_t K, float d, int32_t n_iter, int32_t cand_type, uint32_t excl_edge_mask, "
                "int32_t exclude_self, const int64_t *test_ptr, const int64_t *test_ids, int64_t *pos_out, double *score_out, "
                "int64_t *list_len",
                "GraphHandle g, int[] seeds, int K, float d, int n_iter, int cand_type, uint excl_edge_mask, int exclude_self, "
                "long[] test_ptr, long[] test_ids, long[] pos_out, double[] score_out, long[] list_len"),
        RESTART: ([C.c_void_p, C.c_int32, p(C.c_int64), p(C.c_int32), p(C.c_double), p(C.c_int32), p(C.c_int64), p(C.c_int32),
                   C.c_double, C.c_int32, C.c_int32, C.c_uint32, C.c_int32, p(C.c_int64), p(C.c_int64), p(C.c_int64), p(C.c_double),
                   p(C.c_int64)],
                  "rwr_graph *g, int32_t K, const int64_t *sup_ptr, const int32_t *sup_idx, const double *sup_val, "
                  "const int32_t *start, const int64_t *excl_ptr, const int32_t *excl_idx, double d, int32_t n_iter, "
                  "int32_t cand_type, uint32_t excl_edge_mask, int32_t exclude_members, const int64_t *test_ptr, "
                  "const int64_t *test_ids, int64_t *pos_out, double *score_out, int64_t *list_len",
                  "GraphHandle g, int K, long[] sup_ptr, int[] sup_idx, double[] sup_val, int[] start, long[] excl_ptr, "
                  "int[] excl_idx, double d, int n_iter, int cand_type, uint excl_edge_mask, int exclude_members, long[] test_ptr, "
                  "long[] test_ids, long[] pos_out, double[] score_out, long[] list_len"),
    }
    for name, (argtypes, c_params, cs_params) in want.items():
        assert name in L.EXPORTS
        fn = getattr(lib, name)
        assert fn.restype is C.c_int32 and fn.argtypes == argtypes, name
        m = re.search(r"int32_t\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert m and _flat(m.group(1)) == c_params, name
        m = re.search(r"static extern int %s\(([^)]*)\)" % name, native)
        assert m, "Native.cs does not P/Invoke " + name
        assert " ".join(m.group(1).split()) == cs_params, name
        m = re.search(r"Native\.%s\(([^;]*)\)\);" % name, rec)
        assert m and m.group(1).count(",") + 1 == len(argtypes), name
        assert name in _read("recommendersystems_amd", "csrc", "api.hip")
        for doc in ("INTEGRATION.md", "DESIGN.md", "README.md"):
            assert name in _read(doc), (name, doc)
    for method in ("RecommendationTypedPositionsBatch", "RecommendationTypedPositions", "RecommendationRestartTypedPositionsBatch"):
        assert "public void %s(" % method in rec and method in _read("INTEGRATION.md")
    mk = _read("recommendersystems_amd", "csrc", "Makefile")
    assert "eval_pos.hip" in mk and "eval_pos.h" in mk and "pos_plan.h" in mk
    assert "3.19" in _read("DESIGN.md")
    # the header states the contract: first entry, -1 / +0.0, the caller's order, no top_n
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int32_t %s\(" % TYPED, hdr, re.S)
    doc = " ".join(m.group(1).replace("*", " ").split())
    for words in ("FIRST entry", "-1", "+0.0", "duplicates kept", "best-ranked", "there is no top_n", "A refused call writes nothing"):
        assert words in doc, words


def test_version_string_is_unchanged():
    assert re.search(r'#define\s+RWR_VERSION_STRING\s+"0\.4\.0"', _read("include", "rwr.h"))
    assert _lib().load().rwr_version().startswith(b"0.4.0")


def test_header_is_c99(tmp_path):
    src = tmp_path / "use_rwr.c"
    src.write_text('#include "rwr.h"\n'
                   "int32_t (*a)(rwr_graph *, const int32_t *, int32_t, float, int32_t, int32_t, uint32_t, int32_t, const int64_t *,\n"
                   "             const int64_t *, int64_t *, double *, int64_t *) = %s;\n"
                   "int32_t (*b)(rwr_graph *, int32_t, const int64_t *, const int32_t *, const double *, const int32_t *,\n"
                   "             const int64_t *, const int32_t *, double, int32_t, int32_t, uint32_t, int32_t, const int64_t *,\n"
                   "             const int64_t *, int64_t *, double *, int64_t *) = %s;\n"
                   "int main(void) { return a == 0 || b == 0; }\n" % (TYPED, RESTART))
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I",
                           os.path.join(ROOT, "include"), str(src)])


def test_python_signatures_and_marshalling(monkeypatch):
    from recommendersystems_amd import _lib as L
    from recommendersystems_amd.rwr_based import Recommender, NodeType, EdgeType
    sig = inspect.signature(Recommender.RecommendationTypedPositionsBatch)
    assert list(sig.parameters) == ["self", "seeds", "dampingFactor", "nIteration", "testSets", "candType", "exclEdgeTypes", "excludeSelf"]
    assert sig.parameters["exclEdgeTypes"].default == () and sig.parameters["excludeSelf"].default is False
    sig = inspect.signature(Recommender.RecommendationTypedPositions)
    assert list(sig.parameters) == ["self", "idxTargetNode", "dampingFactor", "nIteration", "testSet", "candType", "exclEdgeTypes",
                                    "excludeSelf"]
    sig = inspect.signature(Recommender.RecommendationRestartTypedPositionsBatch)
    assert list(sig.parameters) == ["self", "restarts", "starts", "dampingFactor", "nIteration", "testSets", "candType", "exclEdgeTypes",
                                    "excludeMembers", "exclude"]
    assert sig.parameters["excludeMembers"].default is False and sig.parameters["exclude"].default is None
    seen = {}

    class FakeLib:
        @staticmethod
        def rwr_recommend_typed_positions_batch(*a):
            K = a[2]
            seen.update(handle=a[0], seeds=[a[1][k] for k in range(K)], K=K, d=a[3].value, T=a[4], cand=a[5], mask=a[6], self_=a[7],
                        ptr=[a[8][k] for k in range(K + 1)])
            seen["ids"] = [a[9][q] for q in range(seen["ptr"][K])]
            for q in range(seen["ptr"][K]):
                a[10][q], a[11][q] = (q if q % 2 == 0 else -1), (0.5 * q if q % 2 == 0 else 0.0)
            for k in range(K):
                a[12][k] = 100 + k
            return 0

        @staticmethod
        def rwr_recommend_restart_typed_positions_batch(*a):
            K = a[1]
            seen.update(K=K, sup=[a[2][k] for k in range(K + 1)], start=None if a[5] is None else [a[5][k] for k in range(K)],
                        eptr=None if a[6] is None else [a[6][k] for k in range(K + 1)], d=a[8], T=a[9], cand=a[10], mask=a[11],
                        members=a[12], ptr=[a[13][k] for k in range(K + 1)])
            for q in range(seen["ptr"][K]):
                a[15][q], a[16][q] = 7 + q, 1.0
            return 0

    class FakeGraph:
        n = 50

        @staticmethod
        def _handle():
            return 1234

    monkeypatch.setattr(L, "load", lambda: FakeLib)
    rec = Recommender.__new__(Recommender)
    rec.graph = FakeGraph
    pos, sc, ln = rec.RecommendationTypedPositionsBatch([3, 9, 3], 0.25, 7, [[12, 11, 12], [], (5,)], NodeType.USER,
                                                        (EdgeType.FRIENDSHIP, EdgeType.FOLLOW), True)
    assert seen["handle"] == 1234 and seen["seeds"] == [3, 9, 3] and seen["K"] == 3 and seen["d"] == 0.25 and seen["T"] == 7
    assert seen["cand"] == int(NodeType.USER) and seen["self_"] == 1
    assert seen["mask"] == (1 << int(EdgeType.FRIENDSHIP)) | (1 << int(EdgeType.FOLLOW))
    assert seen["ptr"] == [0, 3, 3, 4] and seen["ids"] == [12, 11, 12, 5]          # the caller's order, duplicates kept
    assert [p.tolist() for p in pos] == [[0, -1, 2], [], [-1]] and [s.tolist() for s in sc] == [[0.0, 0.0, 1.0], [], [0.0]]
    assert ln.tolist() == [100, 101, 102]
    p1, s1, l1 = rec.RecommendationTypedPositions(3, 0.25, 7, [11, 12], NodeType.ITEM)
    assert seen["K"] == 1 and seen["mask"] == 0 and seen["self_"] == 0 and seen["cand"] == int(NodeType.ITEM)
    assert p1.tolist() == [0, -1] and s1.tolist() == [0.0, 0.0] and l1 == 100
    pos, sc, ln = rec.RecommendationRestartTypedPositionsBatch([{3: 1.0, 5: 2.0}, {7: 0.5}], [3, -1], 0.15, 10, [[1, 2], [3]],
                                                               NodeType.USER, (EdgeType.FOLLOW,), True, exclude=[[3, 3], []])
    assert seen["K"] == 2 and seen["sup"] == [0, 2, 3] and seen["start"] == [3, -1] and seen["eptr"] == [0, 2, 2]
    assert seen["d"] == 0.15 and seen["T"] == 10 and seen["members"] == 1 and seen["mask"] == 1 << int(EdgeType.FOLLOW)
    assert seen["ptr"] == [0, 2, 3] and [p.tolist() for p in pos] == [[7, 8], [9]] and ln.tolist() == [0, 0]
    rec.RecommendationRestartTypedPositionsBatch([{3: 1.0}, {7: 0.5}], None, 0.15, 10, [[], []], NodeType.ITEM)
    assert seen["eptr"] is None and seen["start"] is None and seen["mask"] == 0 and seen["members"] == 0


def test_refusals_before_any_device_work():
    L = _lib()
    lib = L.load()
    seeds = np.array([0, 1], dtype=np.int32)
    tp, ti = np.array([0, 1, 2], dtype=np.int64), np.array([4, 5], dtype=np.int64)
    sup0 = np.zeros(3, dtype=np.int64)                                 # two vectors without support
    sup1, idx, val = np.array([0, 1, 2], dtype=np.int64), np.array([0, 1], dtype=np.int32), np.array([1.0, 1.0])
    pos, sc, ln = np.full(2, -5, dtype=np.int64), np.full(2, -5.0), np.full(2, -5, dtype=np.int64)
    ps, pt, pi = seeds.ctypes.data_as(P32), tp.ctypes.data_as(P64), ti.ctypes.data_as(P64)
    outs = (pos.ctypes.data_as(P64), sc.ctypes.data_as(PD), ln.ctypes.data_as(P64))
    p0, p1, px, pv = sup0.ctypes.data_as(P64), sup1.ctypes.data_as(P64), idx.ctypes.data_as(P32), val.ctypes.data_as(PD)

    def typed(h, s=ps, K=2, cand=1, mask=0x0c, t=(pt, pi), o=outs):
        return getattr(lib, TYPED)(h, s, K, C.c_float(0.15), 3, cand, mask, 1, *t, *o), lib.rwr_last_error()

    def restart(h, K=2, vec=(p0, None, None), cand=1, mask=0x0c, t=(pt, pi), o=outs):
        return getattr(lib, RESTART)(h, K, *vec, None, None, None, 0.15, 3, cand, mask, 1, *t, *o), lib.rwr_last_error()

    # a NULL graph is refused first, whatever else is wrong or missing
    for call, name in ((typed, TYPED), (restart, RESTART)):
        for kw in (dict(), dict(K=0), dict(K=-1), dict(cand=256, mask=1 << 8), dict(t=(None, None), o=(None,) * 3)):
            st, msg = call(None, **kw)
            assert st == L.RWR_E_INVALID and name.encode() in msg and b"NULL graph" in msg, (name, kw, msg)
    fake = C.create_string_buffer(1 << 20)
    h = C.cast(fake, C.c_void_p)
    for call, name in ((typed, TYPED), (restart, RESTART)):
        # K == 0 is a no-op whatever else is wrong; then K, the candidate type and the mask, before the test sets are looked at
        assert call(h, K=0, cand=999, mask=1 << 9, t=(None, None), o=(None,) * 3)[0] == L.RWR_OK
        for kw, word in ((dict(K=-1), b"negative K"), (dict(cand=256), b"cand_type 256"), (dict(cand=-1), b"cand_type"),
                         (dict(mask=1 << 8), b"excl_edge_mask 0x100")):
            for extra in (dict(), dict(t=(None, None)), dict(o=(None,) * 3)):
                st, msg = call(h, **kw, **extra)
                assert st == L.RWR_E_INVALID and name.encode() in msg and word in msg, (name, kw, extra, st, msg)
    # the seeds / the vectors come before the test sets: the stand-in has no nodes, so every seed and index is out of range
    st, msg = typed(h, s=None)
    assert st == L.RWR_E_INVALID and b"seeds" in msg
    st, msg = typed(h, t=(None, None), o=(None,) * 3)
    assert st == L.RWR_E_RANGE and TYPED.encode() in msg and b"batch position 0" in msg
    st, msg = restart(h, vec=(None, None, None))
    assert st == L.RWR_E_INVALID and b"NULL sup_ptr" in msg
    st, msg = restart(h, vec=(p1, px, pv), t=(None, None), o=(None,) * 3)
    assert st == L.RWR_E_RANGE and RESTART.encode() in msg and b"batch position 0" in msg
    # the test sets with pos_out in the place of the result arrays (vectors without support pass on a graph of no nodes)
    name = RESTART.encode()
    for kw, word in ((dict(t=(None, pi)), b"NULL test_ptr"), (dict(o=(None, outs[1], outs[2])), b"NULL pos_out"),
                     (dict(t=(pt, None)), b"NULL test_ids")):
        st, msg = restart(h, **kw)
        assert st == L.RWR_E_INVALID and name in msg and word in msg, (kw, st, msg)
    tp[0] = 1
    st, msg = restart(h)
    assert st == L.RWR_E_INVALID and b"test_ptr[0]" in msg
    tp[:] = [0, 2, 1]
    st, msg = restart(h)
    assert st == L.RWR_E_INVALID and name in msg and b"decreases at batch position 1" in msg
    tp[:] = [0, 1, 2 + 2 ** 31]
    st, msg = restart(h)
    assert st == L.RWR_E_UNSUPPORTED and b"test set 1" in msg
    tp[:] = [0, 1, 2]
    # score_out and list_len may be NULL; the domain comes last
    for o in (outs, (outs[0], None, None)):
        st, msg = restart(h, o=o)
        assert st == L.RWR_E_UNSUPPORTED and name in msg and b"non-negative" in msg, (st, msg)
    assert (pos == -5).all() and (sc == -5.0).all() and (ln == -5).all()      # a refused call writes nothing
