"""What a ranked list among the nodes of another type than ITEM costs: "who to follow" for 256 users of the
synthetic graph -- candidates USER, no edge type excluded, the seed itself left out, T = 10, top-100 --
  (a) by rwr_recommend_typed_batch, and
  (b) by what the library offered before: rwr_model_run_batch into a reused K x n buffer, then a NumPy ranking of every row
      (the USER columns, the seed's own dropped, np.lexsort by score and id, the first 100).
Both in this process on one warmed handle: one warm-up call each, then five timed calls, wall time of the calls (and of the
NumPy ranking) alone; medians and spread.  The lists of the two ways are compared (ids equal, scores bitwise).  A last call of (a)
on a profiling handle gives the phases by the library's own HIP events (rwr_get_stats).

    python tools/typed_latency.py [C2|C4|tiny] [out.jsonl]
"""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from recommendersystems_amd import _lib, synth
from recommendersystems_amd.rwr_based import Graph, NodeType, Recommender, _p

REPS, K, T, TOP_N, D = 5, 256, 10, 100, 0.15
cfg = sys.argv[1] if len(sys.argv) > 1 else "C2"
out_path = sys.argv[2] if len(sys.argv) > 2 else None
no, U, I, E, _ = synth.CONFIGS[cfg]
g = synth.bipartite(no, U, I, E)
flat = {k: g[k] for k in ("node_id", "node_type", "rowptr", "dst", "etype", "w")}
n, m = U + I, int(flat["rowptr"][-1])
lib = _lib.load()
seeds = synth.seeds_for(U, K, 0, K).astype(np.int32)
user_rows = np.flatnonzero(flat["node_type"] == int(NodeType.USER))
user_ids = flat["node_id"][user_rows]
seed_pos = np.searchsorted(user_rows, seeds)                 # (every seed is a user)

G = Graph.from_flat(**flat)
G.buildGraph()
rec = Recommender(G)


def typed():
    return rec.RecommendationTypedBatch(seeds, D, T, TOP_N, NodeType.USER, (), True)


ranks = np.zeros((K, n), dtype=np.float64)                   # the reused buffer of (b)
d_wide = float(np.float32(D))                                # (double)(float)d, as the Recommendation entries widen it


def run_batch():
    _lib.check(lib.rwr_model_run_batch(G._handle(), _p(seeds, C.c_int32), K, d_wide, _lib.RWR_RUN_ITERATIONS, float(T),
                                       _p(ranks, C.c_double), None))


def numpy_rank():
    ids, sc = np.zeros((K, TOP_N), dtype=np.int64), np.zeros((K, TOP_N))
    for k in range(K):
        s = ranks[k, user_rows]
        keep = np.ones(s.shape[0], dtype=bool)
        keep[seed_pos[k]] = False
        s, i = s[keep], user_ids[keep]
        top = np.lexsort((i, s))[::-1][:TOP_N]
        ids[k, :top.shape[0]], sc[k, :top.shape[0]] = i[top], s[top]
    return ids, sc


a = typed()                                                  # warm-up (builds the USER list), and the comparison
run_batch()
b = numpy_rank()
equal = bool((a[0] == b[0]).all() and (a[1].view(np.uint64) == b[1].view(np.uint64)).all() and (a[2] == TOP_N).all())
t_typed, t_run, t_rank = [], [], []
for _ in range(REPS):
    t0 = time.perf_counter()
    typed()
    t_typed.append((time.perf_counter() - t0) * 1e3)
for _ in range(REPS):
    t0 = time.perf_counter()
    run_batch()
    t1 = time.perf_counter()
    numpy_rank()
    t2 = time.perf_counter()
    t_run.append((t1 - t0) * 1e3)
    t_rank.append((t2 - t1) * 1e3)
G.close()

P = Graph.from_flat(**flat, profile=True)                    # the phases of (a), on a handle of its own
P.buildGraph()
recp = Recommender(P)
recp.RecommendationTypedBatch(seeds, D, T, TOP_N, NodeType.USER, (), True)
P.reset_stats()
recp.RecommendationTypedBatch(seeds, D, T, TOP_N, NodeType.USER, (), True)
st = P.stats()
P.close()

r3 = lambda xs: [round(x, 3) for x in xs]
med = lambda xs: float(np.median(xs))
t_b = [x + y for x, y in zip(t_run, t_rank)]
line = dict(config=cfg, n=n, nnz_raw=m, library=lib.rwr_version().decode(), case="typed_who_to_follow", K=K, T=T, top_n=TOP_N,
            candidates=int(user_rows.shape[0]), reps=REPS,
            typed_ms_median=round(med(t_typed), 3), typed_ms_all=r3(t_typed),
            run_batch_ms_median=round(med(t_run), 3), run_batch_ms_all=r3(t_run),
            numpy_rank_ms_median=round(med(t_rank), 3), numpy_rank_ms_all=r3(t_rank),
            run_batch_plus_rank_ms_median=round(med(t_b), 3), speedup_of_medians=round(med(t_b) / med(t_typed), 2),
            faster_beyond_spread=bool(max(t_typed) < min(t_b)), lists_equal=equal,
            bytes_back_typed=int(K * TOP_N * 16 + K * 4), bytes_back_run_batch=int(K * n * 8),
            typed_phases_ms=dict(spmm=round(st["spmm_ms"], 3), chain=round(st["chain_ms"], 3), rank=round(st["rank_ms"], 3),
                                 iterate_wall=round(st["iterate_wall_ms"], 3), total_wall=round(st["total_wall_ms"], 3)),
            tile_seeds=st["tile_seeds"], tile_group=st["tile_group"])
print(json.dumps(line), flush=True)
if out_path:
    with open(out_path, "a") as f:
        f.write(json.dumps(line) + "\n")
