"""What a diversity cap on the ranked lists costs: 256 user seeds of the synthetic graph, T = 10, top-100 ITEM,
the seed's LIKEd items left out.  All in this process on one warmed handle, one warm-up call each, then ten timed calls per
round, two rounds; wall time of the calls alone; medians and every sample.  One line per case and round goes to out.jsonl.
  (a) the identity call -- rwr_recommend_capped_batch with group_of == NULL -- against rwr_recommend_filtered_batch with the
      same arguments, alternating; arrays compared.  With a third argument, the path of ANOTHER build's librwr.so (the parent
      commit's), three child processes of one shape -- a fresh handle, one warm-up call, ten timed calls -- time that
      library's filtered call, this library's filtered call and this library's identity call, and hand back their samples
      and arrays: whether the identity child's median lies inside the spread of the other build's samples is reported as
      measured (like against like: a process that holds one handle and nothing else);
  (b) 5 000 synthetic "authors" of skewed sizes over the items, at most 2 per author, against the only route there was before:
      rwr_model_run_batch into a reused K x n buffer, then NumPy per row -- the liked columns dropped, np.lexsort by score and
      id, the greedy walk as a stable sort by author, the first 100 kept (three timed calls a round: it takes seconds); lists
      compared (ids equal, scores bitwise); the cap stage's own time from rwr_get_stats rank_ms (the library's HIP events) on
      a profiling handle: capped minus filtered;
  (c) ONE group holding every item, at most 1: the longest multi-chunk segment; the cap stage's time the same way.

    python tools/capped_latency.py [C2|C4|tiny] [out.jsonl] [parent librwr.so]
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
if CHILD:                                                    # python tools/capped_latency.py --child <config> <lib> <npz> <call>
    _lib.LIB_PATH = sys.argv[3]

    class _Absent:                                           # (the loader sets prototypes on entries that build does not have)
        pass

    class _OtherBuild(C.CDLL):
        def __getattr__(self, name):
            try:
                return super().__getattr__(name)
            except AttributeError:
                if "capped" in name:
                    return _Absent()
                raise

    C.CDLL = _OtherBuild
from recommendersystems_amd import synth
from recommendersystems_amd.rwr_based import EdgeType, Graph, NodeType, Recommender, _p

REPS, HOST_REPS, ROUNDS, K, T, TOP_N, D, AUTHORS, CAP = 10, 3, 2, 256, 10, 100, 0.15, 5000, 2
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
filtered = lambda r=rec: r.RecommendationFilteredBatch(seeds, D, T, TOP_N, NodeType.ITEM, LIKE, False)

if CHILD:
    call = filtered if sys.argv[5] == "filtered" else (
        lambda: rec.RecommendationCappedBatch(seeds, D, T, TOP_N, NodeType.ITEM, LIKE, False, None, None, None, 0))
    first = call()
    t = [wall(call) for _ in range(REPS)]
    np.savez(sys.argv[4], ids=first[0], scores=first[1], counts=first[2], ms=np.array(t), version=_lib.load().rwr_version().decode())
    G.close()
    sys.exit(0)

lib = _lib.load()
item_rows = np.flatnonzero(flat["node_type"] == int(NodeType.ITEM)).astype(np.int32)
rng = np.random.default_rng(1)
# author sizes ~ 1 / rank: a few prolific authors, a long tail; every item gets one author, in random order over the rows
weights = 1.0 / np.arange(1, AUTHORS + 1)
author_of_item = rng.choice(AUTHORS, item_rows.shape[0], p=weights / weights.sum()).astype(np.int32)
authors = np.full(n, -1, dtype=np.int32)
authors[item_rows] = author_of_item * 7 + 3                  # (labels need not be dense)
one_group = np.full(n, -1, dtype=np.int32)
one_group[item_rows] = 11
liked = [flat["dst"][int(flat["rowptr"][s]):int(flat["rowptr"][s + 1])] for s in seeds]      # (every link of the graph is a LIKE)

identity = lambda r=rec: r.RecommendationCappedBatch(seeds, D, T, TOP_N, NodeType.ITEM, LIKE, False, None, None, None, 0)
capped = lambda r=rec: r.RecommendationCappedBatch(seeds, D, T, TOP_N, NodeType.ITEM, LIKE, False, None, None, authors, CAP)
one = lambda r=rec: r.RecommendationCappedBatch(seeds, D, T, TOP_N, NodeType.ITEM, LIKE, False, None, None, one_group, 1)

ranks = np.zeros((K, n), dtype=np.float64)                   # the reused buffer of (b)
d_wide = float(np.float32(D))                                # (double)(float)d, as the Recommendation entries widen it


def run_batch():
    _lib.check(lib.rwr_model_run_batch(G._handle(), _p(seeds, C.c_int32), K, d_wide, _lib.RWR_RUN_ITERATIONS, float(T),
                                       _p(ranks, C.c_double), None))


def numpy_cap_rank(labels=authors, cap=CAP):
    ids, sc, cnt = np.zeros((K, TOP_N), dtype=np.int64), np.zeros((K, TOP_N)), np.zeros(K, dtype=np.int32)
    for k in range(K):
        r = item_rows[~np.isin(item_rows, liked[k])]
        s, i = ranks[k, r], flat["node_id"][r]
        order = np.lexsort((i, s))[::-1]
        lab = labels[r][order]
        # the greedy walk, vectorised: an entry's count of earlier entries with its label, from a stable sort by label
        by_lab = np.argsort(lab, kind="stable")
        sl = lab[by_lab]
        starts = np.flatnonzero(np.r_[True, sl[1:] != sl[:-1]])
        before = np.empty(lab.shape[0], dtype=np.int64)
        before[by_lab] = np.arange(lab.shape[0]) - np.repeat(starts, np.diff(np.r_[starts, lab.shape[0]]))
        kept = order[(lab < 0) | (before < cap)][:TOP_N]
        cnt[k] = kept.shape[0]
        ids[k, :kept.shape[0]], sc[k, :kept.shape[0]] = i[kept], s[kept]
    return ids, sc, cnt


same = lambda a, b: bool((a[0] == b[0]).all() and (a[1].view(np.uint64) == b[1].view(np.uint64)).all() and (a[2] == b[2]).all())


def emit(line):
    print(json.dumps(line), flush=True)
    if out_path:
        with open(out_path, "a") as f:
            f.write(json.dumps(line) + "\n")


# warm-up of every way, and the comparisons
a_flt, a_ident, a_cap, a_one = filtered(), identity(), capped(), one()
run_batch()
host = numpy_cap_rank()
host_one = numpy_cap_rank(one_group, 1)
identity_equal, capped_equal, one_equal = same(a_flt, a_ident), same(a_cap, host), same(a_one, host_one)
cap_drops = bool((a_cap[0] != a_flt[0]).any())                # the cap is not vacuous on this input

def child(library, call):
    npz = (out_path or "capped_latency") + ".child.npz"
    subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", cfg, library, npz, call])
    z = np.load(npz)
    out = dict(ms=[float(x) for x in z["ms"]], version=str(z["version"]), equal=same(a_ident, (z["ids"], z["scores"], z["counts"])))
    os.remove(npz)
    return out


parent = own_flt = own_ident = None
if parent_lib:
    parent, own_flt, own_ident = child(parent_lib, "filtered"), child(_lib.LIB_PATH, "filtered"), child(_lib.LIB_PATH, "identity")

P = Graph.from_flat(**flat, profile=True)                    # the ranking time of (b) and (c), on a handle of its own
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


sizes = np.bincount(author_of_item, minlength=AUTHORS)
common = dict(config=cfg, n=n, nnz_raw=m, library=lib.rwr_version().decode(), K=K, T=T, top_n=TOP_N, candidates=int(item_rows.shape[0]),
              reps=REPS, cap_chunk=512, tile_seeds=G.stats()["tile_seeds"])
for rnd in range(1, ROUNDS + 1):
    t_flt, t_ident = [], []
    for _ in range(REPS):                                        # alternating: drift hits both alike
        t_flt.append(wall(filtered))
        t_ident.append(wall(identity))
    line = dict(common, case="identity_vs_filtered", round=rnd, filtered_ms_median=round(med(t_flt), 3), filtered_ms_all=r3(t_flt),
                identity_ms_median=round(med(t_ident), 3), identity_ms_all=r3(t_ident),
                identity_minus_filtered_ms=round(med(t_ident) - med(t_flt), 3), arrays_equal=identity_equal)
    if parent:
        line.update(parent_library=parent["version"], child_parent_filtered_ms_all=r3(parent["ms"]),
                    child_parent_filtered_ms_median=round(med(parent["ms"]), 3),
                    child_filtered_ms_all=r3(own_flt["ms"]), child_filtered_ms_median=round(med(own_flt["ms"]), 3),
                    child_identity_ms_all=r3(own_ident["ms"]), child_identity_ms_median=round(med(own_ident["ms"]), 3),
                    child_identity_minus_parent_ms=round(med(own_ident["ms"]) - med(parent["ms"]), 3),
                    child_identity_median_inside_parent_spread=bool(min(parent["ms"]) <= med(own_ident["ms"]) <= max(parent["ms"])),
                    this_process_identity_minus_parent_ms=round(med(t_ident) - med(parent["ms"]), 3),
                    arrays_equal_to_parent=bool(parent["equal"] and own_flt["equal"] and own_ident["equal"]))
    emit(line)
    t_cap = [wall(capped) for _ in range(REPS)]
    t_run, t_host = [], []
    for _ in range(HOST_REPS):                                   # (the host route sorts 500 000 entries per seed: seconds a call)
        t_run.append(wall(run_batch))
        t_host.append(wall(numpy_cap_rank))
    t_b = [x + y for x, y in zip(t_run, t_host)]
    rk_flt, rk_cap, rk_one = rank_ms(filtered), rank_ms(capped), rank_ms(one)
    emit(dict(common, case="authors_5000_cap_2", round=rnd, groups=int((sizes > 0).sum()), largest_group=int(sizes.max()),
              median_group=float(np.median(sizes[sizes > 0])), group_cap=CAP, cap_drops_entries=cap_drops,
              capped_ms_median=round(med(t_cap), 3), capped_ms_all=r3(t_cap),
              run_batch_ms_median=round(med(t_run), 3), run_batch_ms_all=r3(t_run),
              numpy_cap_rank_ms_median=round(med(t_host), 3), numpy_cap_rank_ms_all=r3(t_host),
              run_batch_plus_host_ms_median=round(med(t_b), 3), speedup_of_medians=round(med(t_b) / med(t_cap), 2),
              faster_beyond_spread=bool(max(t_cap) < min(t_b)), lists_equal=capped_equal,
              capped_minus_filtered_ms=round(med(t_cap) - med(t_flt), 3),
              rank_ms_filtered_median=round(med(rk_flt), 3), rank_ms_capped_median=round(med(rk_cap), 3),
              cap_stage_event_ms=round(med(rk_cap) - med(rk_flt), 3), rank_ms_capped_all=r3(rk_cap), rank_ms_filtered_all=r3(rk_flt),
              bytes_in_capped=int(n * 4 + K * 4), bytes_back_capped=int(K * TOP_N * 16 + K * 4), bytes_back_run_batch=int(K * n * 8)))
    t_one = [wall(one) for _ in range(REPS)]
    emit(dict(common, case="one_group_cap_1", round=rnd, group=int(item_rows.shape[0]), group_cap=1,
              chunks=int((item_rows.shape[0] + 511) // 512), one_group_ms_median=round(med(t_one), 3), one_group_ms_all=r3(t_one),
              one_group_minus_filtered_ms=round(med(t_one) - med(t_flt), 3),
              rank_ms_one_group_median=round(med(rk_one), 3), rank_ms_filtered_median=round(med(rk_flt), 3),
              cap_stage_event_ms=round(med(rk_one) - med(rk_flt), 3), rank_ms_one_group_all=r3(rk_one), lists_equal=one_equal))
G.close()
P.close()
