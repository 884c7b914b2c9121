"""What the reasons of ranked entries cost: 256 user seeds of the synthetic graph, T = 10, top-100 ITEM, the
seed's LIKEd items left out, as tools/capped_latency.py sets up.  One warmed handle, one warm-up call each, then ten timed calls
per round, two rounds; wall time of the calls alone; medians and every sample.  One line per case and round goes to out.jsonl.
  (a) the call that asks for nothing -- rwr_recommend_explained_batch with n_why = 0, nodes = NULL, why_total = NULL -- against
      rwr_recommend_capped_batch without labels, alternating; arrays compared.  With a third argument, the path of ANOTHER
      build's librwr.so (the parent commit's), child processes of one shape -- a fresh handle, one warm-up call, ten timed
      calls -- time that library's capped call (twice: its own run-to-run spread) and this library's asks-for-nothing call;
  (b) nodes only: the row-carrying ranking;  (c) n_why = 3;  (d) n_why = 8, each with nodes and why_total.  The extra time over
      (a), and its split: (b) - (a) is the row-carrying collect and sort-and-emit, (c) - (b) and (d) - (b) the reasons kernel
      with its copy-back; rank_ms of a profiling handle (the library's HIP events around the ranked end) gives the same split
      without the copies;
  (e) the host route: rwr_model_run_batch at T and at T - 1 into reused K x n buffers, then NumPy reasons for the same
      entries (three reasons each); lists and reasons compared.
The sum of the in-degrees of the listed entries is reported so that the reasons kernel's gather rate can be read.

    python tools/explained_latency.py [C2|C4|tiny] [out.jsonl] [parent librwr.so]
"""
import ctypes as C
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from recommendersystems_amd import _lib

CHILD = len(sys.argv) > 1 and sys.argv[1] == "--child"
if CHILD:                                                    # python tools/explained_latency.py --child <config> <lib> <npz> <call>
    _lib.LIB_PATH = sys.argv[3]

    class _Absent:                                           # (the loader sets prototypes on entries that build does not have)
        pass

    class _OtherBuild(C.CDLL):
        def __getattr__(self, name):
            try:
                return super().__getattr__(name)
            except AttributeError:
                if "explained" in name:
                    return _Absent()
                raise

    C.CDLL = _OtherBuild
from recommendersystems_amd import synth
from recommendersystems_amd.rwr_based import EdgeType, Graph, NodeType, Recommender, _p

REPS, HOST_REPS, ROUNDS, K, T, TOP_N, D = 10, 3, 2, 256, 10, 100, 0.15
cfg = sys.argv[2] if CHILD else (sys.argv[1] if len(sys.argv) > 1 else "C2")
out_path = None if CHILD else (sys.argv[2] if len(sys.argv) > 2 else None)
parent_lib = None if CHILD else (sys.argv[3] if len(sys.argv) > 3 else None)
no, U, I, E, _ = synth.CONFIGS[cfg]
g = synth.bipartite(no, U, I, E)
flat = {k: g[k] for k in ("node_id", "node_type", "rowptr", "dst", "etype", "w")}
n, m = U + I, int(flat["rowptr"][-1])
seeds = synth.seeds_for(U, K, 0, K).astype(np.int32)
LIKE = (EdgeType.LIKE,)
med = lambda xs: float(np.median(xs))
r3 = lambda xs: [round(x, 3) for x in xs]


def wall(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


G = Graph.from_flat(**flat)
G.buildGraph()
rec = Recommender(G)
capped = lambda r=rec: r.RecommendationCappedBatch(seeds, D, T, TOP_N, NodeType.ITEM, LIKE, False, None, None, None, 0)


def explained(n_why, nodes, total, r=rec):
    return r.RecommendationExplainedBatch(seeds, D, T, TOP_N, n_why, NodeType.ITEM, LIKE, False, None, None, None, 0, nodes, total)


nothing = lambda r=rec: explained(0, False, False, r)
if CHILD:
    call = capped if sys.argv[5] == "capped" else nothing
    first = call()
    t = [wall(call) for _ in range(REPS)]
    np.savez(sys.argv[4], ids=first[0], scores=first[1], counts=first[2], ms=np.array(t), version=_lib.load().rwr_version().decode())
    G.close()
    sys.exit(0)

lib = _lib.load()
rows_only = lambda r=rec: explained(0, True, False, r)
three = lambda r=rec: explained(3, True, True, r)
eight = lambda r=rec: explained(8, True, True, r)
same = lambda a, b: bool((a[0] == b[0]).all() and (a[1].view(np.uint64) == b[1].view(np.uint64)).all() and (a[2] == b[2]).all())

# the host route: two full-vector calls and the in-lists walked in NumPy
ranks_T, ranks_P = np.zeros((K, n), dtype=np.float64), np.zeros((K, n), dtype=np.float64)
d_wide = float(np.float32(D))
c1 = 1 - d_wide
explicit = flat["etype"] != int(EdgeType.UNDEFINED)
src_of = np.repeat(np.arange(n, dtype=np.int32), np.diff(flat["rowptr"]))[explicit]
dst_of = flat["dst"][explicit]
w_sum = np.zeros(n)
np.add.at(w_sum, src_of, flat["w"][explicit])
w_norm = flat["w"][explicit] / w_sum[src_of]
order = np.argsort(dst_of, kind="stable")                    # source ascending, then list position, inside a target
in_src, in_w = src_of[order], w_norm[order]
in_ptr = np.zeros(n + 1, dtype=np.int64)
in_ptr[1:] = np.cumsum(np.bincount(dst_of, minlength=n))
liked = [flat["dst"][int(flat["rowptr"][s]):int(flat["rowptr"][s + 1])] for s in seeds]
item_rows = np.flatnonzero(flat["node_type"] == int(NodeType.ITEM)).astype(np.int32)


def run_two():
    for buf, steps in ((ranks_T, T), (ranks_P, T - 1)):
        _lib.check(lib.rwr_model_run_batch(G._handle(), _p(seeds, C.c_int32), K, d_wide, _lib.RWR_RUN_ITERATIONS, float(steps),
                                           _p(buf, C.c_double), None))


def numpy_reasons(r=3):
    nodes = np.full((K, TOP_N), -1, dtype=np.int32)
    src, term = np.full((K, TOP_N, r), -1, dtype=np.int32), np.zeros((K, TOP_N, r))
    total = np.zeros((K, TOP_N), dtype=np.int64)
    for k in range(K):
        rws = item_rows[~np.isin(item_rows, liked[k])]
        top = rws[np.lexsort((rws, -flat["node_id"][rws], -ranks_T[k, rws]))[:TOP_N]]
        nodes[k, :top.shape[0]] = top
        for j, v in enumerate(top):
            lo, hi = int(in_ptr[v]), int(in_ptr[v + 1])
            a = (c1 * ranks_P[k, in_src[lo:hi]]) * in_w[lo:hi]
            pos = np.flatnonzero(a > 0)
            total[k, j] = pos.shape[0]
            best = pos[np.lexsort((pos, -a[pos]))[:r]]
            src[k, j, :best.shape[0]], term[k, j, :best.shape[0]] = in_src[lo:hi][best], a[best]
    return nodes, src, term, total


def emit(line):
    print(json.dumps(line), flush=True)
    if out_path:
        with open(out_path, "a") as f:
            f.write(json.dumps(line) + "\n")


a_cap, a_nothing, a_rows, a_three, a_eight = capped(), nothing(), rows_only(), three(), eight()
run_two()
host = numpy_reasons()
lists_equal = all(same(a_cap, x) for x in (a_nothing, a_rows, a_three, a_eight))
host_equal = bool((host[0] == a_three[3]).all() and (host[1] == a_three[4]).all() and (host[3] == a_three[6]).all()
                  and (host[2].view(np.uint64) == a_three[5].view(np.uint64)).all())
live = a_three[3] >= 0
in_deg_sum = int((in_ptr[a_three[3][live] + 1] - in_ptr[a_three[3][live]]).sum())


def child(library, call):
    npz = (out_path or "explained_latency") + ".child.npz"
    subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", cfg, library, npz, call])
    z = np.load(npz)
    out = dict(ms=[float(x) for x in z["ms"]], version=str(z["version"]), equal=same(a_cap, (z["ids"], z["scores"], z["counts"])))
    os.remove(npz)
    return out


parent = parent2 = own = None
if parent_lib:
    parent, own, parent2 = child(parent_lib, "capped"), child(_lib.LIB_PATH, "nothing"), child(parent_lib, "capped")

P = Graph.from_flat(**flat, profile=True)                    # the ranked end's own time, on a handle of its own
P.buildGraph()
recp = Recommender(P)


def rank_ms(fn):
    fn(recp)
    out = []
    for _ in range(REPS):
        P.reset_stats()
        fn(recp)
        out.append(P.stats()["rank_ms"])
    return out


common = dict(config=cfg, n=n, nnz_raw=m, library=lib.rwr_version().decode(), K=K, T=T, top_n=TOP_N, candidates=int(item_rows.shape[0]),
              reps=REPS, entries=int(live.sum()), in_degree_sum=in_deg_sum, tile_seeds=G.stats()["tile_seeds"])
for rnd in range(1, ROUNDS + 1):
    t_cap, t_not = [], []
    for _ in range(REPS):                                        # alternating: drift hits both alike
        t_cap.append(wall(capped))
        t_not.append(wall(nothing))
    line = dict(common, case="nothing_vs_capped", round=rnd, capped_ms_median=round(med(t_cap), 3), capped_ms_all=r3(t_cap),
                nothing_ms_median=round(med(t_not), 3), nothing_ms_all=r3(t_not),
                nothing_minus_capped_ms=round(med(t_not) - med(t_cap), 3), arrays_equal=lists_equal)
    if parent:
        line.update(parent_library=parent["version"], child_parent_capped_ms_all=r3(parent["ms"]),
                    child_parent_capped_ms_median=round(med(parent["ms"]), 3),
                    child_parent_capped_again_ms_all=r3(parent2["ms"]), child_parent_capped_again_ms_median=round(med(parent2["ms"]), 3),
                    child_nothing_ms_all=r3(own["ms"]), child_nothing_ms_median=round(med(own["ms"]), 3),
                    child_nothing_minus_parent_ms=round(med(own["ms"]) - med(parent["ms"]), 3),
                    child_nothing_median_inside_parent_spread=bool(min(parent["ms"] + parent2["ms"]) <= med(own["ms"])
                                                                   <= max(parent["ms"] + parent2["ms"])),
                    arrays_equal_to_parent=bool(parent["equal"] and own["equal"] and parent2["equal"]))
    emit(line)
    t_rows, t_3, t_8 = [wall(rows_only) for _ in range(REPS)], [wall(three) for _ in range(REPS)], [wall(eight) for _ in range(REPS)]
    rk_not, rk_rows, rk_3, rk_8 = rank_ms(nothing), rank_ms(rows_only), rank_ms(three), rank_ms(eight)
    emit(dict(common, case="rows_three_eight", round=rnd, rows_only_ms_median=round(med(t_rows), 3), rows_only_ms_all=r3(t_rows),
              three_ms_median=round(med(t_3), 3), three_ms_all=r3(t_3), eight_ms_median=round(med(t_8), 3), eight_ms_all=r3(t_8),
              rows_only_minus_nothing_ms=round(med(t_rows) - med(t_not), 3), three_minus_nothing_ms=round(med(t_3) - med(t_not), 3),
              eight_minus_nothing_ms=round(med(t_8) - med(t_not), 3),
              rank_ms_nothing_median=round(med(rk_not), 3), rank_ms_rows_only_median=round(med(rk_rows), 3),
              rank_ms_three_median=round(med(rk_3), 3), rank_ms_eight_median=round(med(rk_8), 3),
              row_ranking_event_ms=round(med(rk_rows) - med(rk_not), 3), reasons_three_event_ms=round(med(rk_3) - med(rk_rows), 3),
              reasons_eight_event_ms=round(med(rk_8) - med(rk_rows), 3),
              gathered_entries_per_us_three=round(in_deg_sum / max(med(rk_3) - med(rk_rows), 1e-9) / 1e3, 1),
              bytes_back_three=int(K * TOP_N * (16 + 4 + 8 + 3 * 12) + K * 4)))
    t_run, t_host = [], []
    for _ in range(HOST_REPS):
        t_run.append(wall(run_two))
        t_host.append(wall(numpy_reasons))
    t_e = [x + y for x, y in zip(t_run, t_host)]
    emit(dict(common, case="host_route_three", round=rnd, run_batch_twice_ms_median=round(med(t_run), 3), run_batch_twice_ms_all=r3(t_run),
              numpy_reasons_ms_median=round(med(t_host), 3), numpy_reasons_ms_all=r3(t_host),
              host_route_ms_median=round(med(t_e), 3), speedup_of_medians=round(med(t_e) / med(t_3), 2),
              faster_beyond_spread=bool(max(t_3) < min(t_e)), reasons_equal=host_equal, bytes_back_run_batch_twice=int(2 * K * n * 8)))
G.close()
P.close()
