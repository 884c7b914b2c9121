"""rwr_graph_append_links at the C-ABI, in the documents and in the Python mirror's list diff -- checks that need no GPU."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    src = np.array([0, 1], dtype=np.int32)
    dst = np.array([1, 0], dtype=np.int32)
    et = np.array([1, 1], dtype=np.uint8)
    w = np.ones(2)
    out = np.full(2, -7, dtype=np.int64)
    ps, pd = src.ctypes.data_as(C.POINTER(C.c_int32)), dst.ctypes.data_as(C.POINTER(C.c_int32))
    pt, pw = et.ctypes.data_as(C.POINTER(C.c_uint8)), w.ctypes.data_as(C.POINTER(C.c_double))
    po = out.ctypes.data_as(C.POINTER(C.c_int64))
    # a NULL graph is refused first, whatever else is passed
    for count, args in ((2, (ps, pd, pt, pw, po)), (0, (ps, pd, pt, pw, po)), (-1, (ps, pd, pt, pw, po)),
                        (0, (None, None, None, None, None))):
        assert lib.rwr_graph_append_links(None, count, *args) == L.RWR_E_INVALID
        assert b"rwr_graph_append_links" in lib.rwr_last_error()
    # count and the arrays are looked at before the handle is: a block of zeros stands in for one
    fake = C.create_string_buffer(1 << 16)
    h = C.cast(fake, C.c_void_p)
    assert lib.rwr_graph_append_links(h, -1, ps, pd, pt, pw, po) == L.RWR_E_INVALID
    for k in range(4):
        args = [ps, pd, pt, pw]
        args[k] = None
        assert lib.rwr_graph_append_links(h, 2, *args, po) == L.RWR_E_INVALID
        assert b"rwr_graph_append_links" in lib.rwr_last_error()
    assert (out == -7).all()


def test_symbol_prototypes_and_documents():
    L = _lib()
    assert "rwr_graph_append_links" in L.EXPORTS
    fn = L.load().rwr_graph_append_links
    assert fn is not None and len(fn.argtypes) == 7 and fn.restype is C.c_int32
    hdr = _read("include", "rwr.h")
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int32_t rwr_graph_append_links\(rwr_graph \*g, int64_t count, const int32_t \*src, "
                  r"const int32_t \*dst,\s*const uint8_t \*etype, const double \*w,\s*int64_t \*new_index_out[^)]*\);", hdr, re.S)
    assert m, "rwr.h does not declare rwr_graph_append_links with its comment"
    doc = " ".join(m.group(1).replace("*", " ").split())
    # both failure phases, how old positions move, and what is out of scope
    assert "BEFORE THE SWAP" in doc and "RWR_E_NOMEM" in doc and "untouched and usable" in doc
    assert "AFTER THE SWAP" in doc and "invalidates the handle" in doc
    assert "e + (number of appended links with src < i)" in doc
    assert "appending NODES" in doc and "REMOVING links" in doc
    assert re.search(r'#define\s+RWR_VERSION_STRING\s+"0\.4\.0"', hdr)
    native = _read("csharp", "Recommenders", "RWRBased", "Native.cs")
    m = re.search(r"static extern int rwr_graph_append_links\(([^)]*)\)", native)
    assert m and m.group(1).count(",") + 1 == 7
    assert "Native.rwr_graph_append_links(handle," in _read("csharp", "Recommenders", "RWRBased", "Graph.cs")
    hpp = _read("include", "recommenders", "rwr_based.hpp")
    assert "std::vector<int64_t> appendLinks(" in hpp and "rwr_graph_append_links(" in hpp
    rows = [ln for ln in _read("INTEGRATION.md").splitlines() if ln.startswith("|") and "`rwr_graph_append_links`" in ln]
    assert rows, "INTEGRATION.md has no binding-table row for rwr_graph_append_links"
    assert "3.11" in _read("DESIGN.md") and "rwr_graph_append_links" in _read("DESIGN.md")


# ------------------------------------------------------------------------------------------------- the mirror's list diff

def _flatten(node_id, node_type, lists):
    rowptr = np.zeros(len(lists) + 1, dtype=np.int64)
    for i, L in enumerate(lists):
        rowptr[i + 1] = rowptr[i] + len(L)
    flat = [l for L in lists for l in L]
    return (np.array(node_id, dtype=np.int64), np.array(node_type, dtype=np.uint8), rowptr,
            np.array([l[0] for l in flat], dtype=np.int32), np.array([l[1] for l in flat], dtype=np.uint8),
            np.array([l[2] for l in flat], dtype=np.float64))


def _bits(x):
    return np.float64(x).view(np.uint64)


def _brute(old_ids, old_types, old, new_ids, new_types, new):
    """The appended links as (src, dst, etype, weight bits) tuples, or None: list by list, link by link."""
    if list(old_ids) != list(new_ids) or list(old_types) != list(new_types):
        return None
    added = []
    for i, (a, b) in enumerate(zip(old, new)):
        if len(b) < len(a):
            return None
        for x, y in zip(a, b):
            if x[0] != y[0] or x[1] != y[1] or _bits(x[2]) != _bits(y[2]):
                return None
        added += [(i, y[0], y[1], int(_bits(y[2]))) for y in b[len(a):]]
    return added


def test_grown_lists_against_brute_force():
    from recommendersystems_amd.rwr_based import _grown_lists
    rng = np.random.default_rng(77)
    seen = {"growth": 0, "weight": 0, "shorter": 0, "node": 0, "same": 0}
    for case in range(300):
        n = int(rng.integers(1, 12))
        ids = rng.permutation(np.arange(100, 100 + n)).tolist()
        types = rng.integers(0, 4, n).tolist()
        old = [[(int(rng.integers(0, n)), int(rng.integers(0, 8)), float(rng.choice([1.0, 0.5, -0.0, 0.0, 2.0, np.nan])))
                for _ in range(int(rng.integers(0, 5)))] for _ in range(n)]
        new = [list(L) for L in old]
        new_ids, new_types = list(ids), list(types)
        kind = ("growth", "weight", "shorter", "node", "same")[case % 5]
        if kind != "same":
            for _ in range(int(rng.integers(1, 6))):
                new[int(rng.integers(0, n))].append((int(rng.integers(0, n)), int(rng.integers(0, 8)), float(rng.integers(1, 4))))
        if kind == "weight":
            rows = [i for i in range(n) if old[i]]
            if not rows:
                continue
            i = rows[int(rng.integers(0, len(rows)))]
            k = int(rng.integers(0, len(old[i])))
            t, y, wt = new[i][k]
            # (0.0 -> -0.0 compares equal as numbers and differs as bits: it counts as changed)
            new[i][k] = (t, y, -0.0 if _bits(wt) == _bits(0.0) else 0.0 if _bits(wt) == _bits(-0.0) else 7.5)
        if kind == "shorter":
            rows = [i for i in range(n) if old[i]]
            if not rows:
                continue
            i = rows[int(rng.integers(0, len(rows)))]
            new[i] = new[i][:len(old[i]) - 1]
        if kind == "node":
            i = int(rng.integers(0, n))
            new_types[i] = (new_types[i] + 1) % 4
        want = _brute(ids, types, old, new_ids, new_types, new)
        got = _grown_lists(_flatten(ids, types, old), _flatten(new_ids, new_types, new))
        if kind in ("weight", "shorter", "node"):
            assert want is None
        if want is None:
            assert got is None, (case, kind)
        else:
            assert got is not None, (case, kind)
            src, dst, et, w = got
            assert src.dtype == np.int32 and dst.dtype == np.int32 and et.dtype == np.uint8 and w.dtype == np.float64
            assert list(zip(src.tolist(), dst.tolist(), et.tolist(), w.view(np.uint64).tolist())) == want, (case, kind)
            if kind == "same":
                assert src.shape == (0,) and dst.shape == (0,) and et.shape == (0,) and w.shape == (0,)
        seen[kind] += 1
    assert all(v >= 30 for v in seen.values()), seen


def test_merged_flat_against_list_append():
    """What Graph.appendLinks keeps as its record of the device's lists: the old flat lists with the new links at the
    positions the library returns (here: the positions a list-of-lists append gives)."""
    from recommendersystems_amd.rwr_based import _grown_lists, _merged_flat
    rng = np.random.default_rng(91)
    for case in range(100):
        n = int(rng.integers(1, 12))
        ids, types = list(range(n)), rng.integers(0, 4, n).tolist()
        old = [[(int(rng.integers(0, n)), int(rng.integers(0, 8)), float(rng.integers(1, 9))) for _ in range(int(rng.integers(0, 5)))]
               for _ in range(n)]
        count = int(rng.integers(0, 8))
        src = rng.integers(0, n, count).astype(np.int32)
        links = [(int(rng.integers(0, n)), int(rng.integers(0, 8)), float(rng.integers(10, 19)) + 0.001 * q) for q in range(count)]
        new = [list(L) for L in old]
        for q in range(count):
            new[int(src[q])].append(links[q])
        want = _flatten(ids, types, new)
        # position of link q in the new flat list: behind everything of the rows before it and the row's earlier links
        pos = np.array([int(want[2][int(src[q])]) + new[int(src[q])].index(links[q]) for q in range(count)], dtype=np.int64)
        got = _merged_flat(_flatten(ids, types, old), src, np.array([l[0] for l in links], dtype=np.int32),
                           np.array([l[1] for l in links], dtype=np.uint8), np.array([l[2] for l in links], dtype=np.float64), pos)
        assert all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(got, want)), case
        again = _grown_lists(got, want)
        assert again is not None and again[0].shape == (0,)


def test_counter_exists_beside_incremental_rebuilds():
    from recommendersystems_amd.rwr_based import Graph
    assert isinstance(Graph.append_rebuilds, int) and isinstance(Graph.incremental_rebuilds, int)
    assert callable(Graph.appendLinks)
