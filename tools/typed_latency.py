"""What a ranked list among the nodes of another type than ITEM costs: "who to follow" for 256 users of the
synthetic graph -- candidates USER, no edge type excluded, the seed itself left out, T = 10, top-100 --
  (a) by rwr_recommend_typed_batch, and
  (b) by what the library offered before: rwr_model_run_batch into a reused K x n buffer, then a NumPy ranking of every row
      (the USER columns, the seed's own dropped, np.lexsort by score and id, the first 100).
Both in this process on one warmed handle: one warm-up call each, then five timed calls, wall time of the calls (and of the
NumPy ranking) alone; medians and spread.  The lists of the two ways are compared (ids equal, scores bitwise).  A last call of (a)
on a profiling handle gives the phases by the library's own HIP events (rwr_get_stats).

    python tools/typed_latency.py [C2|C4|tiny] [out.jsonl]

With a third argument `eval` the two typed ends of DESIGN §3.17 are measured instead, on the same graph and seeds:
  (a) rwr_recommend_typed_eval_batch, whole USER lists against 50 held-out user ids per seed;
  (b) the only route there was before it: rwr_model_run_batch into a reused buffer, the lexsort ranking above over the whole
      rows, then the harness loop (Experiment.cs:121-128) in NumPy over the whole lists; integers equal, sums bitwise;
  (c) rwr_recommend_typed_batch top-100 again, in the same job;
  (d) rwr_recommend_restart_typed_batch (256 vectors of 8 support users, top-100 users, the members left out) against
      rwr_model_run_restart_batch into a reused buffer plus the host ranking of its rows; lists equal.
One line per pair goes to out.jsonl.

    python tools/typed_latency.py [C2|C4|tiny] [out.jsonl] eval
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
mode = sys.argv[3] if len(sys.argv) > 3 else "rank"
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


r3 = lambda xs: [round(x, 3) for x in xs]
med = lambda xs: float(np.median(xs))


def timed(fn):
    out = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def emit(line):
    print(json.dumps(line), flush=True)
    if out_path:
        with open(out_path, "a") as f:
            f.write(json.dumps(line) + "\n")


def eval_mode():
    rng = np.random.default_rng(1)
    HELD = 50
    tests = [rng.choice(user_ids, min(HELD, user_ids.shape[0]), replace=False) for _ in range(K)]

    def typed_eval():
        return rec.RecommendationTypedEvalBatch(seeds, D, T, tests, NodeType.USER, (), True, 0)

    def numpy_eval():
        hits, sp, ln = np.zeros(K, dtype=np.int64), np.zeros(K), np.zeros(K, dtype=np.int64)
        for k in range(K):
            s = ranks[k, user_rows]
            keep = np.ones(s.shape[0], dtype=bool)
            keep[seed_pos[k]] = False
            s, i = s[keep], user_ids[keep]
            order = np.lexsort((i, s))[::-1]                     # the whole list
            pos = np.flatnonzero(np.isin(i[order], tests[k]))    # ranks of the hits, ascending
            h = pos.shape[0]
            if h:                                                # (double)nHits / (i + 1), summed in rank order
                sp[k] = np.cumsum(np.arange(1, h + 1, dtype=np.float64) / (pos + 1).astype(np.float64))[-1]
            hits[k], ln[k] = h, order.shape[0]
        return hits, sp, ln

    a = typed_eval()                                             # warm-up (builds the USER list), and the comparison
    run_batch()
    b = numpy_eval()
    equal = bool((a[0] == b[0]).all() and (a[2] == b[2]).all() and (a[1].view(np.uint64) == b[1].view(np.uint64)).all())
    typed()
    t_eval, t_typed = timed(typed_eval), timed(typed)
    t_run, t_host = [], []
    for _ in range(REPS):
        t0 = time.perf_counter()
        run_batch()
        t1 = time.perf_counter()
        numpy_eval()
        t2 = time.perf_counter()
        t_run.append((t1 - t0) * 1e3)
        t_host.append((t2 - t1) * 1e3)
    t_b = [x + y for x, y in zip(t_run, t_host)]

    # (d) group walks: 8 support users each, the users ranked, the members left out
    S = 8
    members = [rng.choice(U, S, replace=False).astype(np.int32) for _ in range(K)]
    restarts = [(m, np.full(S, 1.0 / S)) for m in members]
    sup_ptr = (np.arange(K + 1, dtype=np.int64) * S)
    sup_idx = np.ascontiguousarray(np.concatenate(members), dtype=np.int32)
    sup_val = np.full(K * S, 1.0 / S)
    mem_pos = [np.searchsorted(user_rows, m) for m in members]

    def restart_typed():
        return rec.RecommendationRestartTypedBatch(restarts, None, D, T, TOP_N, NodeType.USER, (), True)

    def run_restart_batch():
        _lib.check(lib.rwr_model_run_restart_batch(G._handle(), K, _p(sup_ptr, C.c_int64), _p(sup_idx, C.c_int32),
                                                   _p(sup_val, C.c_double), None, float(D), _lib.RWR_RUN_ITERATIONS, float(T),
                                                   _p(ranks, C.c_double), None))

    def numpy_rank_groups():
        ids, sc = np.zeros((K, TOP_N), dtype=np.int64), np.zeros((K, TOP_N))
        for k in range(K):
            s = ranks[k, user_rows]
            keep = np.ones(s.shape[0], dtype=bool)
            keep[mem_pos[k]] = False
            s, i = s[keep], user_ids[keep]
            top = np.lexsort((i, s))[::-1][:TOP_N]
            ids[k, :top.shape[0]], sc[k, :top.shape[0]] = i[top], s[top]
        return ids, sc

    ra = restart_typed()
    run_restart_batch()
    rb = numpy_rank_groups()
    r_equal = bool((ra[0] == rb[0]).all() and (ra[1].view(np.uint64) == rb[1].view(np.uint64)).all())
    t_rt = timed(restart_typed)
    t_rrun, t_rrank = [], []
    for _ in range(REPS):
        t0 = time.perf_counter()
        run_restart_batch()
        t1 = time.perf_counter()
        numpy_rank_groups()
        t2 = time.perf_counter()
        t_rrun.append((t1 - t0) * 1e3)
        t_rrank.append((t2 - t1) * 1e3)
    t_rb = [x + y for x, y in zip(t_rrun, t_rrank)]
    G.close()

    P = Graph.from_flat(**flat, profile=True)                    # the phases of (a) and (c), on a handle of its own
    P.buildGraph()
    recp = Recommender(P)
    phases = {}
    for name, fn in (("typed_eval", lambda: recp.RecommendationTypedEvalBatch(seeds, D, T, tests, NodeType.USER, (), True, 0)),
                     ("typed_top_n", lambda: recp.RecommendationTypedBatch(seeds, D, T, TOP_N, NodeType.USER, (), True))):
        fn()
        P.reset_stats()
        fn()
        st = P.stats()
        phases[name] = dict(spmm=round(st["spmm_ms"], 3), chain=round(st["chain_ms"], 3), rank=round(st["rank_ms"], 3),
                            iterate_wall=round(st["iterate_wall_ms"], 3), total_wall=round(st["total_wall_ms"], 3))
    tile_seeds, tile_group = st["tile_seeds"], st["tile_group"]
    P.close()

    common = dict(config=cfg, n=n, nnz_raw=m, library=lib.rwr_version().decode(), K=K, T=T, candidates=int(user_rows.shape[0]),
                  reps=REPS, tile_seeds=tile_seeds, tile_group=tile_group)
    emit(dict(common, case="typed_eval_who_to_follow", held_out_per_seed=HELD, top_n=0,
              typed_eval_ms_median=round(med(t_eval), 3), typed_eval_ms_all=r3(t_eval),
              typed_top100_ms_median=round(med(t_typed), 3), typed_top100_ms_all=r3(t_typed),
              eval_minus_top100_ms=round(med(t_eval) - med(t_typed), 3),
              eval_beyond_top100_spread=bool(min(t_eval) > max(t_typed)),
              run_batch_ms_median=round(med(t_run), 3), run_batch_ms_all=r3(t_run),
              numpy_rank_eval_ms_median=round(med(t_host), 3), numpy_rank_eval_ms_all=r3(t_host),
              run_batch_plus_host_ms_median=round(med(t_b), 3), speedup_of_medians=round(med(t_b) / med(t_eval), 2),
              faster_beyond_spread=bool(max(t_eval) < min(t_b)), results_equal=equal,
              hits_total=int(a[0].sum()), list_len_min=int(a[2].min()),
              bytes_in_typed_eval=int(sum(len(t) for t in tests) * 8 + (K + 1) * 8 + K * 4), bytes_back_typed_eval=int(K * 24),
              bytes_back_run_batch=int(K * n * 8), phases_ms=phases))
    emit(dict(common, case="restart_typed_group_follow", support=S, top_n=TOP_N,
              restart_typed_ms_median=round(med(t_rt), 3), restart_typed_ms_all=r3(t_rt),
              run_restart_batch_ms_median=round(med(t_rrun), 3), run_restart_batch_ms_all=r3(t_rrun),
              numpy_rank_ms_median=round(med(t_rrank), 3), numpy_rank_ms_all=r3(t_rrank),
              run_restart_batch_plus_rank_ms_median=round(med(t_rb), 3), speedup_of_medians=round(med(t_rb) / med(t_rt), 2),
              faster_beyond_spread=bool(max(t_rt) < min(t_rb)), lists_equal=r_equal,
              bytes_back_restart_typed=int(K * TOP_N * 16 + K * 4), bytes_back_run_restart_batch=int(K * n * 8)))


if mode == "eval":
    eval_mode()
    sys.exit(0)

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
