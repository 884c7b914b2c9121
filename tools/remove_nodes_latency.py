"""What removing nodes from a resident graph costs: rwr_graph_remove_nodes of 1 / 1 000 / 100 000 random nodes
(four ITEM nodes to one USER node, §3.13's mix) against rwr_graph_destroy + rwr_graph_create with the shortened and renumbered
arrays already flattened on the host.  Both in this process, on a warmed handle (a batch call and a single-seed call ran on
it), five repetitions each, wall time of the calls alone; medians are reported and every sample is kept.  Also recorded: the
re-derive alone of the shortened graph (a call with count 0), the links that left, the bytes of the raw lists and normalised
weights that go with them (21 per link), and a bitwise comparison of the two ways' normalised weights.

    python tools/remove_nodes_latency.py [C2|C4|tiny] [out.jsonl]
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
    # RWR_NODE_REMOVE_TIMING=1 every removal prints wall-clock stamps of its stages to stderr (the times then include the printing)
    _lib.LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), "librwr_exp.so")
from recommendersystems_amd.rwr_based import Graph, Recommender, _p, _removed_nodes_flat

REPS = 5
cfg = sys.argv[1] if len(sys.argv) > 1 else "C2"
out_path = sys.argv[2] if len(sys.argv) > 2 else None
no, U, I, E, K = synth.CONFIGS[cfg]
g = synth.bipartite(no, U, I, E)
KEYS = ("node_id", "node_type", "rowptr", "dst", "etype", "w")
flat = {k: g[k] for k in KEYS}
n, m = U + I, int(flat["rowptr"][-1])
lib = _lib.load()


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
    rng = np.random.default_rng(4000 + count)
    n_users = min(count // 5, U - 1)
    n_items = min(count - n_users, I - 1)
    lost = np.concatenate([rng.permutation(U)[:n_users], U + rng.permutation(I)[:n_items]])
    lost = np.ascontiguousarray(rng.permutation(lost), dtype=np.int32)
    count = int(lost.shape[0])
    after_t, _, new_link = _removed_nodes_flat(tuple(flat[k] for k in KEYS), lost)
    after = {k: np.ascontiguousarray(v) for k, v in zip(KEYS, after_t)}
    links_left = int((new_link < 0).sum())
    del new_link
    t_rem, t_der_dev, t_none, t_destroy_create = [], [], [], []
    same = None
    removed_reported = C.c_int64(-1)
    for rep in range(REPS):
        G = create(flat)
        warm(G)
        t_rem.append(timed(lambda: lib.rwr_graph_remove_nodes(G._handle(), count, _p(lost, C.c_int32), None, None, C.byref(removed_reported))))
        t_der_dev.append(G.stats()["build_ms"])
        t_none.append(timed(lambda: lib.rwr_graph_remove_nodes(G._handle(), 0, None, None, None, None)))   # the re-derive alone
        if rep == 0:                                      # the two ways must leave the same graph
            wa = np.zeros(max(int(after["rowptr"][-1]), 1))
            _lib.check(lib.rwr_graph_get_normalized(G._handle(), _p(wa, C.c_double), None))
        # destroy + create with the shortened arrays, on the same warmed handle's successor
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
    line = dict(config=cfg, n=n, nnz_raw=m, library=lib.rwr_version().decode(), case="graph_remove_nodes", count=count,
                users=int(n_users), items=int(n_items), reps=REPS, links_removed=links_left,
                links_removed_reported=int(removed_reported.value),
                remove_ms_median=med(t_rem), remove_ms_all=r3(t_rem),
                rederive_only_ms_median=med(t_none), rederive_only_ms_all=r3(t_none),
                compaction_ms=round(med(t_rem) - med(t_none), 3), rederive_device_ms_median=med(t_der_dev),
                destroy_create_ms_median=med(t_destroy_create), destroy_create_ms_all=r3(t_destroy_create),
                destroy_create_over_remove=round(med(t_destroy_create) / med(t_rem), 2),
                faster_than_destroy_create_beyond_spread=bool(max(t_rem) < min(t_destroy_create)),
                bytes_given_back=21 * links_left + 9 * count, normalized_bitwise_equal=same)
    print(json.dumps(line), flush=True)
    lines.append(line)
if out_path:
    with open(out_path, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
