"""What the audience of an item costs: top-100 USER audiences of K = 16, 64 and 256 item targets of the synthetic
graph, T = 10, mask {LIKE}.  One warmed handle, one warm-up call each, then ten timed calls per round, two rounds; wall time of
the calls alone; medians and every sample.  One line per case and round goes to out.jsonl.
  (a) the call, for every K;
  (b) its stages by the library's events, on a profiling handle of its own: chain_ms = the restart mass (the dangling column's
      steps and the recurrence), spmm_ms = the reverse steps, rank_ms = the in-link exclusion and the ranked end -- and the
      exclusion alone as the difference of rank_ms between mask {LIKE} and mask 0;
  (c) the yardstick "what a forward call of this size costs": rwr_recommend_typed_batch from 256 user seeds, top-100 ITEM, mask
      {LIKE}, in the same process, and its spmm_ms per step beside the reverse step's;
  (d) the forward route to ONE item's audience: rwr_recommend_typed_positions_batch from a sample of 2 000 users with the item
      as every test set, timed, and that time SCALED to all users (labelled as scaled: it is not measured).

    python tools/audience_latency.py [C2|C4|tiny] [out.jsonl]
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from recommendersystems_amd import _lib
from recommendersystems_amd import synth
from recommendersystems_amd.rwr_based import EdgeType, Graph, NodeType, Recommender

REPS, ROUNDS, KS, T, TOP_N, D, SAMPLE = 10, 2, (16, 64, 256), 10, 100, 0.15, 2000
cfg = sys.argv[1] if len(sys.argv) > 1 else "C2"
out_path = sys.argv[2] if len(sys.argv) > 2 else None
no, U, I, E, _ = synth.CONFIGS[cfg]
g = synth.bipartite(no, U, I, E)
flat = {k: g[k] for k in ("node_id", "node_type", "rowptr", "dst", "etype", "w")}
n, m = U + I, int(flat["rowptr"][-1])
LIKE = (EdgeType.LIKE,)
med = lambda xs: float(np.median(xs))
r3 = lambda xs: [round(x, 3) for x in xs]
in_deg = np.bincount(flat["dst"], minlength=n)
# item targets spread over the in-degree order: heavy and light items
items_by_deg = U + np.argsort(-in_deg[U:], kind="stable")
targets_for = lambda K: items_by_deg[(np.arange(K, dtype=np.int64) * (I // 4)) // K].astype(np.int32)
seeds = synth.seeds_for(U, 256, 0, 256).astype(np.int32)
sample = synth.seeds_for(U, min(SAMPLE, U), 0, min(SAMPLE, U)).astype(np.int32)


def wall(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def emit(line):
    print(json.dumps(line), flush=True)
    if out_path:
        with open(out_path, "a") as f:
            f.write(json.dumps(line) + "\n")


G = Graph.from_flat(**flat)
G.buildGraph()
rec = Recommender(G)
P = Graph.from_flat(**flat, profile=True)
P.buildGraph()
recp = Recommender(P)
aud = lambda r, K, mask=LIKE: r.AudienceBatch(targets_for(K), D, T, NodeType.USER, mask, False, TOP_N)
fwd = lambda r: r.RecommendationTypedBatch(seeds, D, T, TOP_N, NodeType.ITEM, LIKE, False)
one_item = int(targets_for(16)[3])
route = lambda r: r.RecommendationTypedPositionsBatch(sample, D, T, [[int(flat["node_id"][one_item])]] * len(sample), NodeType.ITEM,
                                                      LIKE, False)


def stages(fn):
    fn(recp)
    out = {"chain_ms": [], "spmm_ms": [], "rank_ms": [], "iterate_wall_ms": [], "spmm_launches": 0}
    for _ in range(REPS):
        P.reset_stats()
        fn(recp)
        st = P.stats()
        for k in ("chain_ms", "spmm_ms", "rank_ms", "iterate_wall_ms"):
            out[k].append(st[k])
        out["spmm_launches"] = st["spmm_launches"]
    return out


common = dict(config=cfg, n=n, users=U, nnz_raw=m, library=_lib.load().rwr_version().decode(), T=T, top_n=TOP_N, reps=REPS,
              max_out_degree=int(np.diff(flat["rowptr"]).max()), max_in_degree=int(in_deg.max()))
for K in KS:
    aud(rec, K)
fwd(rec)
route(rec)
for rnd in range(1, ROUNDS + 1):
    t_fwd = [wall(lambda: fwd(rec)) for _ in range(REPS)]
    s_fwd = stages(fwd)
    fwd_step = med(s_fwd["spmm_ms"]) / max(s_fwd["spmm_launches"], 1)
    emit(dict(common, case="forward_typed_yardstick", round=rnd, K=256, ms_median=round(med(t_fwd), 3), ms_all=r3(t_fwd),
              spmm_ms_median=round(med(s_fwd["spmm_ms"]), 3), spmm_launches=int(s_fwd["spmm_launches"]),
              spmm_ms_per_launch=round(fwd_step, 3), rank_ms_median=round(med(s_fwd["rank_ms"]), 3)))
    for K in KS:
        t = [wall(lambda: aud(rec, K)) for _ in range(REPS)]
        s1, s0 = stages(lambda r: aud(r, K)), stages(lambda r: aud(r, K, ()))
        step = med(s1["spmm_ms"]) / max(s1["spmm_launches"], 1)
        emit(dict(common, case="audience", round=rnd, K=K, tile_seeds=G.stats()["tile_seeds"], ms_median=round(med(t), 3), ms_all=r3(t),
                  rho_ms_median=round(med(s1["chain_ms"]), 3), steps_ms_median=round(med(s1["spmm_ms"]), 3),
                  step_launches=int(s1["spmm_launches"]), ms_per_step=round(step, 3),
                  exclusion_and_ranked_end_ms_median=round(med(s1["rank_ms"]), 3),
                  ranked_end_ms_median=round(med(s0["rank_ms"]), 3),
                  exclusion_ms_by_difference=round(med(s1["rank_ms"]) - med(s0["rank_ms"]), 3),
                  rho_share_of_call=round(med(s1["chain_ms"]) / med(t), 4),
                  reverse_step_over_forward_step_K256=round(step / fwd_step, 3) if K == 256 else None))
    t_route = [wall(lambda: route(rec)) for _ in range(3)]
    emit(dict(common, case="forward_route_one_item", round=rnd, sample_users=int(len(sample)), ms_median=round(med(t_route), 3),
              ms_all=r3(t_route), scaled_to_all_users_ms=round(med(t_route) * U / len(sample), 1),
              note="scaled_to_all_users_ms is the sample's time times users / sample, not a measurement"))
G.close()
P.close()
