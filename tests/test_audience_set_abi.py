"""The audience set entries (rwr_recommend_audience_set_batch, rwr_recommend_audience_set_positions_batch) at the C-ABI and in the
host mirrors -- checks that need no GPU.  The order, the status and the message of every refusal beyond the handle are
audience_set_plan.h's: the compiled check program (tests/test_audience_set_plan.py) prints them for a call that holds every
fault at once, one step repaired at a time; here they are compared with the order the header states, and the NULL graph is
shown to come first at the library itself."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

from tests.test_audience_set_plan import build_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LISTS, POSITIONS = "rwr_recommend_audience_set_batch", "rwr_recommend_audience_set_positions_batch"
HEAD = ("rwr_graph *g, int32_t K, const int64_t *set_ptr, const int32_t *set_idx, const double *set_w, float d, int32_t n_iter, "
        "int32_t cand_type, uint32_t etype_mask, int32_t exclude_members, int32_t n_pool, const int32_t *pool_idx, "
        "const int64_t *deny_ptr, const int32_t *deny_idx, ")
C_DECL = {LISTS: HEAD + "int32_t top_n, int64_t *out_id, double *out_score, int32_t *out_node, int32_t *out_count",
          POSITIONS: HEAD + "const int64_t *test_ptr, const int64_t *test_ids, int64_t *out_pos, double *out_score, int64_t *out_len"}
CS_HEAD = ("GraphHandle g, int K, long[] set_ptr, int[] set_idx, double[] set_w, float d, int n_iter, int cand_type, uint etype_mask, "
           "int exclude_members, int n_pool, int[] pool_idx, long[] deny_ptr, int[] deny_idx, ")
CS_DECL = {LISTS: CS_HEAD + "int top_n, long[] out_id, double[] out_score, int[] out_node, int[] out_count",
           POSITIONS: CS_HEAD + "long[] test_ptr, long[] test_ids, long[] out_pos, double[] out_score, long[] out_len"}
INVALID, RANGE, UNSUPPORTED = 1, 2, 7


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
    head = [C.c_void_p, C.c_int32, p(C.c_int64), p(C.c_int32), p(C.c_double), C.c_float, C.c_int32, C.c_int32, C.c_uint32, C.c_int32,
            C.c_int32, p(C.c_int32), p(C.c_int64), p(C.c_int32)]
    want = {LISTS: head + [C.c_int32, p(C.c_int64), p(C.c_double), p(C.c_int32), p(C.c_int32)],
            POSITIONS: head + [p(C.c_int64), p(C.c_int64), p(C.c_int64), p(C.c_double), p(C.c_int64)]}
    hdr = _read("include", "rwr.h")
    native = _read("csharp", "Recommenders", "RWRBased", "Native.cs")
    rec = _read("csharp", "Recommenders", "RWRBased", "Recommender.cs")
    hpp = _read("include", "recommenders", "rwr_based.hpp")
    for name in (LISTS, POSITIONS):
        assert name in L.EXPORTS
        fn = getattr(lib, name)
        assert fn.restype is C.c_int32 and fn.argtypes == want[name] and len(want[name]) == 19
        m = re.search(r"int32_t\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert m and _flat(m.group(1)) == C_DECL[name]
        m = re.search(r"static extern int %s\(([^)]*)\)" % name, native)
        assert m and " ".join(m.group(1).split()) == CS_DECL[name]
        m = re.search(r"Native\.%s\(([^;]*)\)\);" % name, rec)
        assert m and re.sub(r"\([^()]*\)", "", m.group(1)).count(",") + 1 == 19
        assert name + "(" in hpp and name in _read("recommendersystems_amd", "csrc", "api.hip")
        for doc in ("INTEGRATION.md", "DESIGN.md", "README.md"):
            assert name in _read(doc), doc
    for method in ("AudienceSetBatch(", "AudienceSet(", "AudienceSetPositionsBatch("):
        assert "public " in rec and method in rec, method
        assert method[:-1] in _read("INTEGRATION.md"), method
    for method in ("audienceSetBatch(", "audienceSet(", "audienceSetPositionsBatch("):
        assert method in hpp
    mk = _read("recommendersystems_amd", "csrc", "Makefile")
    assert "audience_set_plan.h" in mk
    assert "3.26" in _read("DESIGN.md")


def test_header_states_the_contract_and_the_ladders_order():
    hdr = _read("include", "rwr.h")
    doc = " ".join(hdr[hdr.index("The audience of a weighted target SET"):hdr.index("int32_t %s(" % LISTS)].replace("\n *", " ").split())
    for word in ("a_v * x_T^(s)[v]", "added on the host, in list order", "ANY member", "exclude_members", "ONE pool", "n_pool == 0",
                 "deny list k", "bitwise what rwr_recommend_audience_batch returns", "does not depend on K", "no floating-point atomics",
                 "struck out", "tol_rel = 8 * (n_iter + 1) * (n + L + m + 8) * 2^-53 / d", "+0.0", "[2^-256, 2^256]", "writes nothing",
                 "RWR_E_INVALID", "RWR_E_RANGE", "RWR_E_UNSUPPORTED", "negative weights"):
        assert word in doc, word
    order = [doc.index(w) for w in ("g NULL or a poisoned handle", "K < 0", "set_ptr[0] != 0", "set_ptr decreasing", "an empty set",
                                    "a NULL set_idx", "the first member outside [0, n) or weight", "top_n outside [1, 1024]", "n_iter < 0",
                                    "cand_type outside", "n_pool > 0 with a NULL pool_idx", "a pool index outside", "the deny lists as",
                                    "the domain (RWR_E_UNSUPPORTED)", "then K == 0 succeeds")]
    assert order == sorted(order)
    doc = " ".join(hdr[hdr.index("int32_t %s(" % LISTS):hdr.index("int32_t %s(" % POSITIONS)].replace("\n *", " ").split())
    for word in ("WHOLE audience lists", "first entry of list k with that id", "-1 / +0.0", "out_len[k] is the list's length",
                 "the test sets as rwr_recommend_filtered_positions_batch reports them"):
        assert word in doc, word
    # the single-target entry's comment names only what is still open
    aud = " ".join(hdr[hdr.index("The audience of an item"):hdr.index("int32_t rwr_recommend_audience_batch(")].replace("\n *", " ").split())
    assert "Answered by rwr_recommend_audience_set_batch" in aud and "- Not here: duals" not in aud


def test_every_refusal_has_its_status_and_message_in_the_documented_order(tmp_path):
    exe = build_check(tmp_path, sanitize=False)
    out = subprocess.run([str(exe), "messages"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    common = [(INVALID, "NULL graph"), (INVALID, "negative K"), (INVALID, "NULL set_ptr"), (INVALID, "set_ptr[0] = 2, not 0"),
              (INVALID, "set_ptr decreases at batch position 1"), (INVALID, "set 1 is empty"), (INVALID, "NULL set_idx"),
              (RANGE, "member 6 (set 2, position 0) is outside [0, 6)"), (RANGE, "(set 2, position 0) is not a finite number in [2^-256, 2^256]"),
              (RANGE, "top_n 1025 is outside [1, 1024]"), (INVALID, "n_iter -1 is negative"), (INVALID, "cand_type 256 is outside [-1, 255]"),
              (INVALID, "etype_mask 0x100 has a bit beyond the 8 edge types"), (INVALID, "NULL pool_idx"),
              (RANGE, "pool index -1 (pool position 1) is outside [0, 6)"), (INVALID, "deny_ptr[0] = 1, not 0"),
              (INVALID, "deny_ptr decreases at batch position 1"), (INVALID, "NULL deny_idx"),
              (RANGE, "deny index 6 (batch position 1) is outside [0, 6)")]
    tests = [(INVALID, "NULL test_ptr"), (INVALID, "NULL out_pos"), (INVALID, "test_ptr[0] = 1, not 0"),
             (INVALID, "test_ptr decreases at batch position 1"), (INVALID, "NULL test_ids"), (UNSUPPORTED, "test set 1 holds more than INT32_MAX ids")]
    want = [(LISTS,) + x for x in common] + [(POSITIONS,) + x for x in common if "top_n" not in x[1]] + [(POSITIONS,) + x for x in tests]
    lines = out.stdout.strip().split("\n")
    assert len(lines) == len(want) == 19 + 18 + 6
    last = 0
    for line, (who, status, word) in zip(lines, want):
        verdict, st, text = line.split(" ", 2)
        assert int(st) == status and text.startswith(who + ": ") and word in text, (line, status, word)
        assert int(verdict) > last or who == POSITIONS and int(verdict) == 1   # ascending: the enum is the ladder
        last = int(verdict)
    assert "out_id, out_score or out_count" in lines[2] and "out_id" not in lines[19 + 2]


def test_header_is_c99(tmp_path):
    src = tmp_path / "use_rwr.c"
    src.write_text('#include "rwr.h"\n'
                   "int32_t (*fa)(rwr_graph *, int32_t, const int64_t *, const int32_t *, const double *, float, int32_t, int32_t, uint32_t,\n"
                   "              int32_t, int32_t, const int32_t *, const int64_t *, const int32_t *, int32_t, int64_t *, double *, int32_t *,\n"
                   "              int32_t *) = %s;\n"
                   "int32_t (*fb)(rwr_graph *, int32_t, const int64_t *, const int32_t *, const double *, float, int32_t, int32_t, uint32_t,\n"
                   "              int32_t, int32_t, const int32_t *, const int64_t *, const int32_t *, const int64_t *, const int64_t *,\n"
                   "              int64_t *, double *, int64_t *) = %s;\n"
                   "int main(void) { return fa == 0 || fb == 0; }\n" % (LISTS, POSITIONS))
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I",
                           os.path.join(ROOT, "include"), str(src)])


def test_null_graph_is_refused_first():
    L = _lib()
    lib = L.load()
    PI32, PI64, PD = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)
    sp, si, sw = np.array([0, 1, 1], dtype=np.int64), np.array([99], dtype=np.int32), np.array([np.nan])
    ids, sc = np.full((2, 3), -5, dtype=np.int64), np.full((2, 3), -5.0)
    nodes, cnt = np.full((2, 3), -5, dtype=np.int32), np.full(2, -5, dtype=np.int32)
    pos, ln = np.full(2, -5, dtype=np.int64), np.full(2, -5, dtype=np.int64)
    a = (sp.ctypes.data_as(PI64), si.ctypes.data_as(PI32), sw.ctypes.data_as(PD))
    for K, sets, T, cand, mask, npool in ((2, a, 3, 1, 2, -1), (0, a, 3, -1, 0, -1), (-1, a, 3, 1, 0, 5), (2, (None,) * 3, -4, 999, 0xffff, 7)):
        assert lib.rwr_recommend_audience_set_batch(None, K, *sets, C.c_float(7.5), T, cand, mask, 1, npool, None, None, None, 0,
                                                    ids.ctypes.data_as(PI64), sc.ctypes.data_as(PD), nodes.ctypes.data_as(PI32),
                                                    cnt.ctypes.data_as(PI32)) == L.RWR_E_INVALID
        msg = lib.rwr_last_error()
        assert LISTS.encode() + b": NULL graph" in msg
        assert lib.rwr_recommend_audience_set_positions_batch(None, K, *sets, C.c_float(7.5), T, cand, mask, 1, npool, None, None, None,
                                                              None, None, pos.ctypes.data_as(PI64), sc.ctypes.data_as(PD),
                                                              ln.ctypes.data_as(PI64)) == L.RWR_E_INVALID
        msg = lib.rwr_last_error()
        assert POSITIONS.encode() + b": NULL graph" in msg
    for x in (ids, sc, nodes, cnt, pos, ln):
        assert (x == -5).all()


def test_python_mirror_marshals_as_declared(monkeypatch):
    from recommendersystems_amd import _lib as L
    from recommendersystems_amd.rwr_based import Recommender, NodeType, EdgeType
    sig = inspect.signature(Recommender.AudienceSetBatch)
    assert list(sig.parameters) == ["self", "sets", "d", "n_iter", "weights", "cand_type", "etype_mask", "exclude_members", "pool", "deny", "top_n"]
    assert sig.parameters["weights"].default is None and sig.parameters["pool"].default is None and sig.parameters["top_n"].default == 100
    assert list(inspect.signature(Recommender.AudienceSet).parameters)[1] == "members"
    assert list(inspect.signature(Recommender.AudienceSetPositionsBatch).parameters)[:5] == ["self", "sets", "d", "n_iter", "testSets"]
    seen = {}

    def common(a):
        K = a[1]
        total = a[2][K]
        seen.update(handle=a[0], K=K, ptr=[a[2][k] for k in range(K + 1)], idx=[a[3][q] for q in range(total)],
                    w=None if not a[4] else [a[4][q] for q in range(total)], d=a[5].value, T=a[6], cand=a[7], mask=a[8], members=a[9],
                    n_pool=a[10], pool=None if a[10] < 0 else [a[11][q] for q in range(a[10])],
                    deny=None if not a[12] else ([a[12][k] for k in range(K + 1)], [a[13][q] for q in range(a[12][K])]))
        return K

    class FakeLib:
        @staticmethod
        def rwr_recommend_audience_set_batch(*a):
            K, top = common(a), a[14]
            seen.update(top=top)
            for k in range(K):
                a[15][k * top], a[16][k * top], a[17][k * top], a[18][k] = 70 + k, 0.5 + k, 40 + k, 1
            return 0

        @staticmethod
        def rwr_recommend_audience_set_positions_batch(*a):
            K = common(a)
            seen.update(tests=([a[14][k] for k in range(K + 1)], [a[15][q] for q in range(a[14][K])]))
            for q in range(a[14][K]):
                a[16][q], a[17][q] = q, 0.25 * q
            for k in range(K):
                a[18][k] = 9 + k
            return 0

    class FakeGraph:
        @staticmethod
        def _handle():
            return 1234

    monkeypatch.setattr(L, "load", lambda: FakeLib)
    rec = Recommender.__new__(Recommender)
    rec.graph = FakeGraph
    ids, sc, nodes, cnt = rec.AudienceSetBatch([[9, 3, 9], [4]], 0.25, 7, [[1.0, 0.25, 3.7], [2.0]], NodeType.USER,
                                               (EdgeType.LIKE, EdgeType.UNDEFINED), True, [5, 1, 5], [[], [8, 2]], 4)
    assert seen["handle"] == 1234 and seen["K"] == 2 and seen["ptr"] == [0, 3, 4] and seen["idx"] == [9, 3, 9, 4]
    assert seen["w"] == [1.0, 0.25, 3.7, 2.0] and seen["d"] == 0.25 and seen["T"] == 7 and seen["cand"] == int(NodeType.USER)
    assert seen["mask"] == (1 << int(EdgeType.LIKE)) | (1 << int(EdgeType.UNDEFINED)) and seen["members"] == 1
    assert seen["n_pool"] == 3 and seen["pool"] == [5, 1, 5] and seen["deny"] == ([0, 0, 2], [8, 2]) and seen["top"] == 4
    assert ids.shape == (2, 4) and ids[:, 0].tolist() == [70, 71] and sc[:, 0].tolist() == [0.5, 1.5]
    assert nodes.dtype == np.int32 and nodes[:, 0].tolist() == [40, 41] and nodes[0, 1] == -1 and cnt.tolist() == [1, 1]
    # the defaults: no weights, any type, no mask, no pool, no deny lists; an empty pool; a mask given as a number
    rec.AudienceSetBatch([np.array([5, 2], dtype=np.int32)], 0.5, 0)
    assert seen["idx"] == [5, 2] and seen["w"] is None and seen["cand"] == -1 and seen["mask"] == 0 and seen["members"] == 0
    assert seen["n_pool"] == -1 and seen["deny"] is None and seen["top"] == 100
    rec.AudienceSetBatch([[1]], 0.5, 0, pool=[], etype_mask=0x06)
    assert seen["n_pool"] == 0 and seen["pool"] == [] and seen["mask"] == 6
    assert rec.AudienceSet([3, 6], 0.25, 7, [0.25, 1.0], NodeType.ITEM, deny=[7], top_n=2) == [(70, 0.5)]
    assert seen["K"] == 1 and seen["idx"] == [3, 6] and seen["w"] == [0.25, 1.0] and seen["deny"] == ([0, 1], [7]) and seen["top"] == 2
    pos, psc, ln = rec.AudienceSetPositionsBatch([[9, 3], [4]], 0.25, 7, [[11, 12, 11], []], [[1.0, 0.25], [3.7]], NodeType.USER, 2, True,
                                                 [5], [[1], []])
    assert seen["tests"] == ([0, 3, 3], [11, 12, 11]) and seen["idx"] == [9, 3, 4] and seen["w"] == [1.0, 0.25, 3.7] and seen["mask"] == 2
    assert seen["pool"] == [5] and seen["deny"] == ([0, 1, 1], [1])
    assert [p.tolist() for p in pos] == [[0, 1, 2], []] and [s.tolist() for s in psc] == [[0.0, 0.25, 0.5], []] and ln.tolist() == [9, 10]
