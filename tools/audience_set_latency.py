"""What the audience of a weighted target set costs: top-100 USER audiences on the synthetic graph, T = 10, mask
{LIKE}.  One warmed handle, one warm-up call each, then ten timed calls per round, two rounds; wall time of the calls alone;
medians and every sample (their min - max is the spread).  One line per case and round goes to out.jsonl.
  (i)   16 unit one-member sets through rwr_recommend_audience_set_batch against rwr_recommend_audience_batch for the same
        targets, alternating in one process; "single" runs the second alone, for a fresh process on this or on another commit;
  (ii)  16 sets of 100 item members against rwr_recommend_audience_batch with K = 1 600 (the members as targets, top_n 1 024)
        plus the host merge of every set's 100 lists -- which is exact only where no list was cut;
  (iii) the same 16 sets with a pool of 10 % of the users and 500 denied users per set, against the call without them;
  (iv)  rwr_recommend_audience_set_positions_batch for 50 held-out likers per set against the ranked call.
Stages by the library's events come from a profiling handle of its own.

    python tools/audience_set_latency.py [C2|C4|tiny] [out.jsonl] [all|single]
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

REPS, ROUNDS, T, TOP_N, D, KSETS, MEMBERS, DENIED, HELD = 10, 2, 10, 100, 0.15, 16, 100, 500, 50
cfg = sys.argv[1] if len(sys.argv) > 1 else "C2"
out_path = sys.argv[2] if len(sys.argv) > 2 else None
what = sys.argv[3] if len(sys.argv) > 3 else "all"
no, U, I, E, _ = synth.CONFIGS[cfg]
g = synth.bipartite(no, U, I, E)
flat = {k: g[k] for k in ("node_id", "node_type", "rowptr", "dst", "etype", "w")}
n, m = U + I, int(flat["rowptr"][-1])
LIKE = (EdgeType.LIKE,)
med = lambda xs: float(np.median(xs))
r3 = lambda xs: [round(x, 3) for x in xs]
rng = np.random.default_rng(326)
in_deg = np.bincount(flat["dst"], minlength=n)
items_by_deg = U + np.argsort(-in_deg[U:], kind="stable")
targets = items_by_deg[(np.arange(KSETS, dtype=np.int64) * (I // 4)) // KSETS].astype(np.int32)   # tools/audience_latency.py's K = 16
members = min(MEMBERS, I // KSETS)
sets = [np.sort(rng.choice(np.arange(U, n), size=members, replace=False)).astype(np.int32) for _ in range(KSETS)]
weights = [rng.choice([0.25, 1.0, 3.7], size=members) for _ in range(KSETS)]
pool = rng.choice(U, size=max(U // 10, 1), replace=False).astype(np.int32)
deny = [rng.choice(U, size=min(DENIED, U), replace=False).astype(np.int32) for _ in range(KSETS)]
# held-out likers: sources of links into the set's members (they are excluded by the mask, so they answer -1: the counting is the same)
src_of = np.repeat(np.arange(n, dtype=np.int64), np.diff(flat["rowptr"]))
tests = []
for s in sets:
    likers = np.unique(src_of[np.isin(flat["dst"], s)])
    pick = likers[:HELD // 2].tolist() + rng.choice(U, size=HELD - min(HELD // 2, len(likers)), replace=False).tolist()
    tests.append([int(flat["node_id"][u]) for u in pick])


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
single = lambda r: r.AudienceBatch(targets, D, T, NodeType.USER, LIKE, False, TOP_N)
unit = lambda r: r.AudienceSetBatch([[int(v)] for v in targets], D, T, None, NodeType.USER, LIKE, False, None, None, TOP_N)
ranked = lambda r, p=None, dn=None: r.AudienceSetBatch(sets, D, T, weights, NodeType.USER, LIKE, False, p, dn, TOP_N)
positions = lambda r: r.AudienceSetPositionsBatch(sets, D, T, tests, weights, NodeType.USER, LIKE, False, None, None)
flat_members = np.concatenate(sets).astype(np.int32)
flat_weights = np.concatenate(weights)


def merged_route(r):
    """K x |set| single-target lists at the ranked entry's widest top_n, then the host merge; exact only where no list was cut"""
    ids, sc, nodes, cnt = r.AudienceBatch(flat_members, D, T, NodeType.USER, (), False, 1024)
    t0 = time.perf_counter()
    cut = int((cnt == 1024).sum())
    for k in range(KSETS):
        acc = np.zeros(n)
        for j in range(k * members, (k + 1) * members):
            c = int(cnt[j])
            np.add.at(acc, nodes[j, :c], flat_weights[j] * sc[j, :c])
        np.argpartition(-acc[:U], TOP_N)[:TOP_N]
    return (time.perf_counter() - t0) * 1e3, cut


def stages(fn):
    fn(recp)
    out = {"chain_ms": [], "spmm_ms": [], "rank_ms": [], "iterate_wall_ms": []}
    for _ in range(REPS):
        P.reset_stats()
        fn(recp)
        st = P.stats()
        for k in out:
            out[k].append(st[k])
    return {k + "_median": round(med(v), 3) for k, v in out.items()}


common = dict(config=cfg, n=n, users=U, nnz_raw=m, library=_lib.load().rwr_version().decode(), T=T, top_n=TOP_N, reps=REPS, sets=KSETS,
              members=members)
if what == "single":
    single(rec)
    for rnd in range(1, ROUNDS + 1):
        t = [wall(lambda: single(rec)) for _ in range(REPS)]
        emit(dict(common, case="i_audience_batch_fresh_process", round=rnd, ms_median=round(med(t), 3), ms_min=round(min(t), 3),
                  ms_max=round(max(t), 3), ms_all=r3(t)))
    G.close()
    sys.exit(0)

P = Graph.from_flat(**flat, profile=True)
P.buildGraph()
recp = Recommender(P)
a, b = single(rec), unit(rec)
equal = all((np.ascontiguousarray(x).view(np.uint8) == np.ascontiguousarray(y).view(np.uint8)).all() for x, y in zip(a, b))
ranked(rec), ranked(rec, pool, deny), positions(rec)
for rnd in range(1, ROUNDS + 1):
    ta, tb = [], []
    for _ in range(REPS):                                        # alternating
        ta.append(wall(lambda: single(rec)))
        tb.append(wall(lambda: unit(rec)))
    emit(dict(common, case="i_unit_sets_against_audience_batch", round=rnd, arrays_equal=bool(equal), audience_ms_median=round(med(ta), 3),
              audience_ms_all=r3(ta), unit_sets_ms_median=round(med(tb), 3), unit_sets_ms_all=r3(tb),
              audience_stages=stages(single), unit_sets_stages=stages(unit)))
    t = [wall(lambda: ranked(rec)) for _ in range(REPS)]
    emit(dict(common, case="ii_sets_of_members", round=rnd, ms_median=round(med(t), 3), ms_all=r3(t), stages=stages(ranked)))
    t_call, t_merge, cut = [], [], 0
    for _ in range(3):
        t0 = time.perf_counter()
        mm, cut = merged_route(rec)
        t_call.append((time.perf_counter() - t0) * 1e3 - mm)
        t_merge.append(mm)
    emit(dict(common, case="ii_single_target_route", round=rnd, K=int(len(flat_members)), reps=3, call_ms_median=round(med(t_call), 3),
              call_ms_all=r3(t_call), host_merge_ms_median=round(med(t_merge), 3), host_merge_ms_all=r3(t_merge),
              lists_cut_at_1024=cut, note="the merge is exact only where no list was cut"))
    t = [wall(lambda: ranked(rec, pool, deny)) for _ in range(REPS)]
    emit(dict(common, case="iii_pool_and_deny", round=rnd, pool=int(len(pool)), denied_per_set=int(len(deny[0])), ms_median=round(med(t), 3),
              ms_all=r3(t), stages=stages(lambda r: ranked(r, pool, deny))))
    t = [wall(lambda: positions(rec)) for _ in range(REPS)]
    emit(dict(common, case="iv_positions", round=rnd, test_ids_per_set=HELD, ms_median=round(med(t), 3), ms_all=r3(t),
              stages=stages(positions)))
G.close()
P.close()
