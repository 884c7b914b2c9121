"""What removing links from a resident graph costs: rwr_graph_remove_links of 1 / 1 000 / 100 000 random LIKE links
against the two things the library offered before for the same edit --
  (a) rwr_graph_destroy + rwr_graph_create with the shortened arrays already flattened on the host;
  (b) the documented workaround: rwr_graph_update_links relabelling the same positions to UNDEFINED (the links stay).
All three in this process, on a warmed handle (a batch call and a single-seed call ran on it), five repetitions each, wall time
of the calls alone; medians are reported and every sample is kept.  The normalised weights of the removal and of (a) are
compared bitwise in every count, and the bytes the removal gives back are stated (13 per link in the raw lists, 8 more in the
per-link normalised weights).

    python tools/remove_latency.py [C2|C4|tiny] [out.jsonl]
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
    # RWR_REMOVE_TIMING=1 every removal prints wall-clock stamps of its stages to stderr (the times then include the printing)
    _lib.LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), "librwr_exp.so")
from recommendersystems_amd.rwr_based import Graph, Recommender, _p

REPS = 5
EDGE_UNDEFINED, EDGE_LIKE = 0, 1
cfg = sys.argv[1] if len(sys.argv) > 1 else "C2"
out_path = sys.argv[2] if len(sys.argv) > 2 else None
no, U, I, E, K = synth.CONFIGS[cfg]
g = synth.bipartite(no, U, I, E)
flat = {k: g[k] for k in ("node_id", "node_type", "rowptr", "dst", "etype", "w")}
n, m = U + I, int(flat["rowptr"][-1])
lib = _lib.load()
likes = np.flatnonzero(flat["etype"] == EDGE_LIKE)


def shortened(f, pos):
    """the flattened lists after the removal, on the host"""
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(f["rowptr"]))
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(np.delete(src, pos), minlength=n), out=rowptr[1:])
    return dict(node_id=f["node_id"], node_type=f["node_type"], rowptr=rowptr, dst=np.ascontiguousarray(np.delete(f["dst"], pos)),
                etype=np.ascontiguousarray(np.delete(f["etype"], pos)), w=np.ascontiguousarray(np.delete(f["w"], pos)))


def create(f):
    G = Graph.from_flat(**f)
    G.buildGraph()
    return G


def warm(G):
    Recommender(G).RecommendationBatch(synth.seeds_for(U, 64, 0, 64), 0.15, 3, 10)
    Recommender(G).RecommendationArrays(0, 0.15, 3, 10)


def timed(call):
    t = time.perf_counter()
    _lib.check(call())
    return (time.perf_counter() - t) * 1e3


lines = []
for count in (1, 1000, 100000):
    rng = np.random.default_rng(3000 + count)
    pos = np.ascontiguousarray(rng.permutation(likes)[:min(count, likes.shape[0])], dtype=np.int64)
    count = int(pos.shape[0])
    after = shortened(flat, pos)
    undefined = np.full(count, EDGE_UNDEFINED, dtype=np.uint8)
    t_rem, t_der_dev, t_none, t_relabel, t_destroy_create = [], [], [], [], []
    same = None
    for rep in range(REPS):
        # (b) the workaround, on a warmed handle that holds the whole graph
        G = create(flat)
        warm(G)
        t_relabel.append(timed(lambda: lib.rwr_graph_update_links(G._handle(), count, _p(pos, C.c_int64), _p(undefined, C.c_uint8), None)))
        G.close()
        # the removal, on another such handle
        G = create(flat)
        warm(G)
        t_rem.append(timed(lambda: lib.rwr_graph_remove_links(G._handle(), count, _p(pos, C.c_int64))))
        t_der_dev.append(G.stats()["build_ms"])
        t_none.append(timed(lambda: lib.rwr_graph_remove_links(G._handle(), 0, None)))   # the re-derive alone, of the shortened graph
        if rep == 0:                                      # the two ways must leave the same graph
            wa = np.zeros(max(int(after["rowptr"][-1]), 1))
            _lib.check(lib.rwr_graph_get_normalized(G._handle(), _p(wa, C.c_double), None))
        # (a) destroy + create with the shortened arrays, on the same warmed handle's successor
        t = time.perf_counter()
        G.close()
        H = Graph.from_flat(**after)
        H.buildGraph()
        t_destroy_create.append((time.perf_counter() - t) * 1e3)
        if rep == 0:
            wb = np.zeros(max(int(after["rowptr"][-1]), 1))
            _lib.check(lib.rwr_graph_get_normalized(H._handle(), _p(wb, C.c_double), None))
            same = bool(np.array_equal(wa.view(np.uint64), wb.view(np.uint64)))
        H.close()
    med = lambda xs: round(float(np.median(xs)), 3)
    r3 = lambda xs: [round(x, 3) for x in xs]
    line = dict(config=cfg, n=n, nnz_raw=m, library=lib.rwr_version().decode(), case="graph_remove", count=count, reps=REPS,
                remove_ms_median=med(t_rem), remove_ms_all=r3(t_rem),
                rederive_only_ms_median=med(t_none), rederive_only_ms_all=r3(t_none),
                compaction_ms=round(med(t_rem) - med(t_none), 3), rederive_device_ms_median=med(t_der_dev),
                destroy_create_ms_median=med(t_destroy_create), destroy_create_ms_all=r3(t_destroy_create),
                relabel_ms_median=med(t_relabel), relabel_ms_all=r3(t_relabel),
                destroy_create_over_remove=round(med(t_destroy_create) / med(t_rem), 2),
                relabel_over_remove=round(med(t_relabel) / med(t_rem), 2),
                faster_than_destroy_create_beyond_spread=bool(max(t_rem) < min(t_destroy_create)),
                bytes_given_back=21 * count, normalized_bitwise_equal=same)
    print(json.dumps(line), flush=True)
    lines.append(line)
if out_path:
    with open(out_path, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
