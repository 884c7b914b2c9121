"""What one edit of a resident graph costs: rwr_graph_append_links of 1 / 1 000 / 100 000 random LIKE links against
what the library offered before for the same edit -- rwr_graph_destroy + rwr_graph_create with the patched arrays already
flattened on the host.  Both in this process, on a warmed handle, best of 5, wall time of the calls alone.  The append call
splits into the re-derive (an append of NOTHING to the patched graph right afterwards, wall time; and its device time by the
library's own HIP events, rwr_stats.build_ms) and the merge (plan, upload, device merge), which is reported as the DIFFERENCE of
the two best wall times: below about 0.1 ms that difference is noise, not a measurement.

    python tools/append_latency.py [C2|C4|tiny] [out.jsonl] [links|nodes]

nodes mode: rwr_graph_append_nodes of 1 000 / 100 000 new nodes -- four in five a new ITEM with one LIKE from a
random user, the fifth a new USER with three LIKEs -- against destroy + create with the grown arrays, measured in the same run:
five repetitions each, reported as median and spread (min .. max), and the links-only re-derive of the grown graph beside them.
"""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from recommendersystems_amd import _lib, synth
if os.environ.get("RWR_TOOLS_EXP_LIB"):        # the experiments build (make -C recommendersystems_amd/csrc exp): with
    # RWR_APPEND_TIMING=1 every append call prints wall-clock stamps of its stages to stderr (the times above then include the printing)
    _lib.LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), "librwr_exp.so")
from recommendersystems_amd.rwr_based import Graph, Recommender, _p

REPS = 5
cfg = sys.argv[1] if len(sys.argv) > 1 else "C2"
out_path = sys.argv[2] if len(sys.argv) > 2 else None
no, U, I, E, K = synth.CONFIGS[cfg]
g = synth.bipartite(no, U, I, E)
flat = {k: g[k] for k in ("node_id", "node_type", "rowptr", "dst", "etype", "w")}
n, m = U + I, int(flat["rowptr"][-1])
lib = _lib.load()


def patched(f, src, dst, et, w):
    """the flattened lists after the append, on the host (stable sort by source: link q at the end of list src[q])"""
    all_src = np.concatenate([np.repeat(np.arange(n, dtype=np.int64), np.diff(f["rowptr"])), src.astype(np.int64)])
    order = np.argsort(all_src, kind="stable")
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(all_src, minlength=n), out=rowptr[1:])
    return dict(node_id=f["node_id"], node_type=f["node_type"], rowptr=rowptr,
                dst=np.ascontiguousarray(np.concatenate([f["dst"], dst])[order]),
                etype=np.ascontiguousarray(np.concatenate([f["etype"], et])[order]),
                w=np.ascontiguousarray(np.concatenate([f["w"], w])[order]))


def create(f):
    G = Graph.from_flat(**f)
    G.buildGraph()
    return G


def warm(G):
    Recommender(G).RecommendationBatch(synth.seeds_for(U, 64, 0, 64), 0.15, 3, 10)
    Recommender(G).RecommendationArrays(0, 0.15, 3, 10)


def append_ms(G, src, dst, et, w):
    t = time.perf_counter()
    _lib.check(lib.rwr_graph_append_links(G._handle(), int(src.shape[0]), _p(src, C.c_int32), _p(dst, C.c_int32), _p(et, C.c_uint8),
                                          _p(w, C.c_double), None))
    dt = (time.perf_counter() - t) * 1e3
    return dt, G.stats()["build_ms"]


def nodes_mode():
    out = []
    for n_new in (1000, 100000):
        rng = np.random.default_rng(2000 + n_new)
        is_user = np.arange(n_new) % 5 == 4
        new_type = np.where(is_user, flat["node_type"][0], flat["node_type"][n - 1]).astype(np.uint8)   # (users first, items last)
        new_id = (int(flat["node_id"].max()) + 1 + rng.permutation(n_new)).astype(np.int64)
        rows = (n + np.arange(n_new)).astype(np.int32)
        items, users = rows[~is_user], rows[is_user]
        src = np.concatenate([rng.integers(0, U, items.shape[0]).astype(np.int32), np.repeat(users, 3)])
        dst = np.concatenate([items, rng.integers(U, n, 3 * users.shape[0]).astype(np.int32)])
        count = int(src.shape[0])
        et, w = np.ones(count, dtype=np.uint8), np.ones(count)
        nt = n + n_new
        all_src = np.concatenate([np.repeat(np.arange(n, dtype=np.int64), np.diff(flat["rowptr"])), src.astype(np.int64)])
        order = np.argsort(all_src, kind="stable")
        rowptr = np.zeros(nt + 1, dtype=np.int64)
        np.cumsum(np.bincount(all_src, minlength=nt), out=rowptr[1:])
        after = dict(node_id=np.concatenate([flat["node_id"], new_id]), node_type=np.concatenate([flat["node_type"], new_type]),
                     rowptr=rowptr, dst=np.ascontiguousarray(np.concatenate([flat["dst"], dst])[order]),
                     etype=np.ascontiguousarray(np.concatenate([flat["etype"], et])[order]),
                     w=np.ascontiguousarray(np.concatenate([flat["w"], w])[order]))
        t_app, t_none, t_dc = [], [], []
        same = None
        for rep in range(REPS):
            G = create(flat)
            warm(G)
            t = time.perf_counter()
            _lib.check(lib.rwr_graph_append_nodes(G._handle(), n_new, _p(new_id, C.c_int64), _p(new_type, C.c_uint8), count,
                                                  _p(src, C.c_int32), _p(dst, C.c_int32), _p(et, C.c_uint8), _p(w, C.c_double), None))
            t_app.append((time.perf_counter() - t) * 1e3)
            t = time.perf_counter()
            _lib.check(lib.rwr_graph_append_links(G._handle(), 0, None, None, None, None, None))   # the re-derive alone
            t_none.append((time.perf_counter() - t) * 1e3)
            if rep == 0:
                wa, da = np.zeros(int(rowptr[-1])), np.zeros(nt, dtype=np.uint8)
                _lib.check(lib.rwr_graph_get_normalized(G._handle(), _p(wa, C.c_double), _p(da, C.c_uint8)))
                G._flat, G._n, G._rowptr = tuple(after[k] for k in ("node_id", "node_type", "rowptr", "dst", "etype", "w")), nt, rowptr
                la = Recommender(G).RecommendationArrays(0, 0.15, 3, 50)
            t = time.perf_counter()
            G.close()
            H = Graph.from_flat(**after)
            H.buildGraph()
            t_dc.append((time.perf_counter() - t) * 1e3)
            if rep == 0:
                wb, db = np.zeros(int(rowptr[-1])), np.zeros(nt, dtype=np.uint8)
                _lib.check(lib.rwr_graph_get_normalized(H._handle(), _p(wb, C.c_double), _p(db, C.c_uint8)))
                lb = Recommender(H).RecommendationArrays(0, 0.15, 3, 50)
                same = bool(np.array_equal(wa.view(np.uint64), wb.view(np.uint64)) and np.array_equal(da, db)
                            and np.array_equal(la[0], lb[0]) and np.array_equal(la[1].view(np.uint64), lb[1].view(np.uint64)))
            H.close()
        r3 = lambda xs: [round(x, 3) for x in xs]
        line = dict(config=cfg, n=n, nnz_raw=m, library=lib.rwr_version().decode(), case="graph_append_nodes", n_new=n_new,
                    new_items=int(items.shape[0]), new_users=int(users.shape[0]), count=count, reps=REPS,
                    append_nodes_ms_median=round(float(np.median(t_app)), 3), append_nodes_ms_min=round(min(t_app), 3),
                    append_nodes_ms_max=round(max(t_app), 3), append_nodes_ms_all=r3(t_app),
                    rederive_only_ms_median=round(float(np.median(t_none)), 3), rederive_only_ms_all=r3(t_none),
                    destroy_create_ms_median=round(float(np.median(t_dc)), 3), destroy_create_ms_min=round(min(t_dc), 3),
                    destroy_create_ms_max=round(max(t_dc), 3), destroy_create_ms_all=r3(t_dc),
                    speedup_of_medians=round(float(np.median(t_dc)) / float(np.median(t_app)), 2),
                    faster_beyond_spread=bool(max(t_app) < min(t_dc)), results_bitwise_equal=same)
        print(json.dumps(line), flush=True)
        out.append(line)
    if out_path:
        with open(out_path, "a") as f:
            for line in out:
                f.write(json.dumps(line) + "\n")


if len(sys.argv) > 3 and sys.argv[3] == "nodes":
    nodes_mode()
    sys.exit(0)

lines = []
for count in (1, 1000, 100000):
    rng = np.random.default_rng(1000 + count)
    src = rng.integers(0, U, count).astype(np.int32)
    dst = rng.integers(U, n, count).astype(np.int32)
    et = np.ones(count, dtype=np.uint8)
    w = np.ones(count)
    after = patched(flat, src, dst, et, w)
    none = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.uint8), np.zeros(0))
    t_app, t_der_dev, t_none, t_create, t_destroy_create = [], [], [], [], []
    same = None
    for rep in range(REPS):
        # the append, on a warmed handle that holds the unpatched graph
        G = create(flat)
        warm(G)
        a, d = append_ms(G, src, dst, et, w)
        t_app.append(a)
        t_der_dev.append(d)
        t_none.append(append_ms(G, *none)[0])             # nothing to merge: the re-derive alone, of the same (patched) graph
        if rep == 0:                                      # the two ways must leave the same graph
            wa = np.zeros(int(after["rowptr"][-1]))
            _lib.check(lib.rwr_graph_get_normalized(G._handle(), _p(wa, C.c_double), None))
        # destroy + create with the patched arrays, on the same warmed handle's successor
        t = time.perf_counter()
        G.close()
        H = Graph.from_flat(**after)
        H.buildGraph()
        t_destroy_create.append((time.perf_counter() - t) * 1e3)
        if rep == 0:
            wb = np.zeros(int(after["rowptr"][-1]))
            _lib.check(lib.rwr_graph_get_normalized(H._handle(), _p(wb, C.c_double), None))
            same = bool(np.array_equal(wa.view(np.uint64), wb.view(np.uint64)))
        H.close()
    line = dict(config=cfg, n=n, nnz_raw=m, library=lib.rwr_version().decode(), case="graph_append", count=count, reps=REPS,
                append_ms=round(min(t_app), 3), append_ms_all=[round(x, 3) for x in t_app],
                rederive_only_ms=round(min(t_none), 3), merge_ms=round(min(t_app) - min(t_none), 3),
                rederive_device_ms=round(min(t_der_dev), 3),
                destroy_create_ms=round(min(t_destroy_create), 3), destroy_create_ms_all=[round(x, 3) for x in t_destroy_create],
                speedup=round(min(t_destroy_create) / min(t_app), 2), normalized_bitwise_equal=same)
    print(json.dumps(line), flush=True)
    lines.append(line)
if out_path:
    with open(out_path, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
