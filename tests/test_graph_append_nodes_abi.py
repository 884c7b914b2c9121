"""rwr_graph_append_nodes at the C-ABI, in the documents and in the Python mirror's dictionary diff -- checks that need no GPU."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C_PARAMS = ["rwr_graph *g", "int32_t n_new", "const int64_t *node_id", "const uint8_t *node_type", "int64_t count",
            "const int32_t *src", "const int32_t *dst", "const uint8_t *etype", "const double *w", "int64_t *new_index_out"]


def _lib():
    import __graft_entry__ as ge
    from recommendersystems_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_argument_errors_without_gpu():
    L = _lib()
    lib = L.load()
    nid = np.array([7, 8], dtype=np.int64)
    nty = np.array([1, 0], dtype=np.uint8)
    src = np.array([0, 1], dtype=np.int32)
    dst = np.array([1, 0], dtype=np.int32)
    et = np.array([1, 1], dtype=np.uint8)
    w = np.ones(2)
    out = np.full(2, -7, dtype=np.int64)
    pi, py = nid.ctypes.data_as(C.POINTER(C.c_int64)), nty.ctypes.data_as(C.POINTER(C.c_uint8))
    ps, pd = src.ctypes.data_as(C.POINTER(C.c_int32)), dst.ctypes.data_as(C.POINTER(C.c_int32))
    pt, pw = et.ctypes.data_as(C.POINTER(C.c_uint8)), w.ctypes.data_as(C.POINTER(C.c_double))
    po = out.ctypes.data_as(C.POINTER(C.c_int64))
    # a NULL graph is refused first, whatever else is passed
    for n_new, count in ((2, 2), (0, 0), (-1, 0), (0, -1)):
        assert lib.rwr_graph_append_nodes(None, n_new, pi, py, count, ps, pd, pt, pw, po) == L.RWR_E_INVALID
        assert b"rwr_graph_append_nodes" in lib.rwr_last_error()
    # the counts and the arrays are looked at before the handle is: a block of zeros stands in for one
    fake = C.create_string_buffer(1 << 16)
    h = C.cast(fake, C.c_void_p)
    assert lib.rwr_graph_append_nodes(h, -1, pi, py, 2, ps, pd, pt, pw, po) == L.RWR_E_INVALID
    assert lib.rwr_graph_append_nodes(h, 2, pi, py, -1, ps, pd, pt, pw, po) == L.RWR_E_INVALID
    assert lib.rwr_graph_append_nodes(h, 2, None, py, 0, None, None, None, None, None) == L.RWR_E_INVALID
    assert lib.rwr_graph_append_nodes(h, 2, pi, None, 0, None, None, None, None, None) == L.RWR_E_INVALID
    for k in range(4):
        args = [ps, pd, pt, pw]
        args[k] = None
        assert lib.rwr_graph_append_nodes(h, 2, pi, py, 2, *args, po) == L.RWR_E_INVALID
        assert lib.rwr_graph_append_nodes(h, 0, None, None, 2, *args, po) == L.RWR_E_INVALID
        assert b"rwr_graph_append_nodes" in lib.rwr_last_error()
    assert (out == -7).all()


def test_symbol_prototypes_and_documents():
    L = _lib()
    assert "rwr_graph_append_nodes" in L.EXPORTS
    fn = L.load().rwr_graph_append_nodes
    assert fn is not None and fn.restype is C.c_int32
    p = C.POINTER
    assert list(fn.argtypes) == [C.c_void_p, C.c_int32, p(C.c_int64), p(C.c_uint8), C.c_int64, p(C.c_int32), p(C.c_int32),
                                 p(C.c_uint8), p(C.c_double), p(C.c_int64)]
    hdr = _read("include", "rwr.h")
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int32_t rwr_graph_append_nodes\(([^)]*)\);", hdr, re.S)
    assert m, "rwr.h does not declare rwr_graph_append_nodes with its comment"
    params = [" ".join(a.split()) for a in re.sub(r"/\*.*?\*/", "", m.group(2)).split(",")]
    assert params == C_PARAMS, params
    doc = " ".join(m.group(1).replace("*", " ").split())
    assert "index n + j" in doc and "bit for bit" in doc and "rank[seed] = n + n_new" in doc
    assert "n_new == 0 is rwr_graph_append_links" in doc and "count == 0 is legal" in doc
    assert "RWR_E_NOMEM" in doc and "invalidates the handle" in doc and "INT32_MAX" in doc
    assert "rwr_part_begin" in doc and "REMOVING or renumbering nodes" in doc and "anywhere but at the end" in doc
    # the links-only entry points at this one
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int32_t rwr_graph_append_links\(", hdr, re.S)
    assert m and "rwr_graph_append_nodes" in m.group(1) and "create a new graph" not in m.group(1)
    # the C# declaration: the same parameters in the same order
    native = _read("csharp", "Recommenders", "RWRBased", "Native.cs")
    m = re.search(r"static extern int rwr_graph_append_nodes\(([^)]*)\)", native)
    assert m
    cs = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert cs == ["GraphHandle g", "int n_new", "long[] node_id", "byte[] node_type", "long count", "int[] src", "int[] dst",
                  "byte[] etype", "double[] w", "long[] new_index_out"]
    assert [c.split()[-1] for c in cs] == [a.replace("*", " ").split()[-1] for a in C_PARAMS]
    graph_cs = _read("csharp", "Recommenders", "RWRBased", "Graph.cs")
    assert graph_cs.count("Native.rwr_graph_append_nodes(handle,") == 2 and "public long[] AppendNodes(" in graph_cs
    assert "NodeAppendRebuilds" in graph_cs
    rows = [ln for ln in _read("INTEGRATION.md").splitlines() if ln.startswith("|") and "`rwr_graph_append_nodes`" in ln]
    assert rows, "INTEGRATION.md has no binding-table row for rwr_graph_append_nodes"
    design = _read("DESIGN.md")
    assert "3.13" in design and "rwr_graph_append_nodes" in design and "k_item_order_merge" in design


def test_header_stays_plain_c(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "rwr.h"\nint32_t (*fp)(rwr_graph *, int32_t, const int64_t *, const uint8_t *, int64_t, const int32_t *,\n'
                   '               const int32_t *, const uint8_t *, const double *, int64_t *) = rwr_graph_append_nodes;\n'
                   'int main(void) { return fp == 0; }\n')
    import subprocess
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-c", "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(tmp_path / "use.o")])


# ------------------------------------------------------------------------------------------- the mirror's dictionary diff

def _flatten(node_id, node_type, lists):
    rowptr = np.zeros(len(lists) + 1, dtype=np.int64)
    for i, L in enumerate(lists):
        rowptr[i + 1] = rowptr[i] + len(L)
    flat = [l for L in lists for l in L]
    return (np.array(node_id, dtype=np.int64), np.array(node_type, dtype=np.uint8), rowptr,
            np.array([l[0] for l in flat], dtype=np.int32), np.array([l[1] for l in flat], dtype=np.uint8),
            np.array([l[2] for l in flat], dtype=np.float64))


def test_grown_nodes_against_brute_force():
    from recommendersystems_amd.rwr_based import _extended_flat, _grown_nodes, _merged_flat
    rng = np.random.default_rng(1313)
    seen = {"grown": 0, "old node": 0, "old link": 0, "no node": 0}
    for case in range(240):
        n = int(rng.integers(1, 10))
        k = int(rng.integers(1, 6))
        ids = rng.integers(-50, 50, n + k).tolist()
        types = rng.integers(0, 4, n + k).tolist()
        old = [[(int(rng.integers(0, n)), int(rng.integers(0, 8)), float(rng.integers(1, 5))) for _ in range(int(rng.integers(0, 4)))]
               for _ in range(n)]
        new = [list(L) for L in old] + [[] for _ in range(k)]
        added = []
        for _ in range(int(rng.integers(0, 9))):
            s = int(rng.integers(0, n + k))
            link = (int(rng.integers(0, n + k)), int(rng.integers(0, 8)), float(rng.integers(5, 9)))
            new[s].append(link)
        for i, L in enumerate(new):
            added += [(i,) + l for l in L[len(old[i]) if i < n else 0:]]
        kind = ("grown", "old node", "old link", "no node")[case % 4]
        new_ids, new_types = list(ids), list(types)
        if kind == "old node":
            i = int(rng.integers(0, n))
            if rng.random() < 0.5:
                new_ids[i] += 1
            else:
                new_types[i] = (new_types[i] + 1) % 4
        if kind == "old link":
            rows = [i for i in range(n) if old[i]]
            if not rows:
                continue
            i = rows[int(rng.integers(0, len(rows)))]
            t, y, wt = new[i][0]
            new[i][0] = (t, y, wt + 0.5)
        old_flat = _flatten(ids[:n], types[:n], old)
        if kind == "no node":
            assert _grown_nodes(old_flat, _flatten(new_ids[:n], new_types[:n], new[:n])) is None
            seen[kind] += 1
            continue
        got = _grown_nodes(old_flat, _flatten(new_ids, new_types, new))
        if kind != "grown":
            assert got is None, (case, kind)
        else:
            assert got is not None and got[0] == n, case
            src, dst, et, w = got[1]
            assert src.dtype == np.int32 and dst.dtype == np.int32 and et.dtype == np.uint8 and w.dtype == np.float64
            assert list(zip(src.tolist(), dst.tolist(), et.tolist(), w.tolist())) == added, case
            # the record Graph.appendNodes keeps: extended, then merged at the positions a list append gives
            want = _flatten(ids, types, new)
            pos = np.flatnonzero(np.isin(np.arange(want[3].shape[0]),
                                         [int(want[2][i]) + j for i, L in enumerate(new)
                                          for j in range(len(old[i]) if i < n else 0, len(L))])).astype(np.int64)
            ext = _extended_flat(old_flat, np.array(ids[n:], dtype=np.int64), np.array(types[n:], dtype=np.uint8))
            rec = _merged_flat(ext, src, dst, et, w, pos)
            assert all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(rec, want)), case
        seen[kind] += 1
    assert all(v >= 40 for v in seen.values()), seen


def test_counter_and_method_exist():
    from recommendersystems_amd.rwr_based import Graph
    assert isinstance(Graph.node_append_rebuilds, int) and isinstance(Graph.append_rebuilds, int)
    assert callable(Graph.appendNodes)
