"""Restart-vector walks evaluated on the device (rwr_recommend_restart_eval_batch) against the only route there was before
it -- the numbers of DESIGN §3.15.  tools/restart_rank_time.py's batch on a BASELINE-config graph (default C2): K in {64, 256}
vectors of |S| = 8 random support rows (the hub row in one of them), every vector from the global constructor's rank, T = 10,
d = 0.15f, the default exclusion sets, 50 held-out item ids per vector.  Timed in the same run, on one handle warmed with the
same batch, best of 3 (all three repetitions are recorded):
  (a) rwr_recommend_restart_eval_batch with top_n = 0;
  (b) rwr_recommend_restart_batch with top_n = n_items into buffers touched beforehand, plus the host evaluation of its lists
      with numpy (membership, hit positions, the addends summed left to right); call and host part timed separately;
  (c) rwr_recommend_restart_batch at top-100: the cost of the walk with a cheap end.
The results of (a) must equal (b)'s (integers equal, sums bitwise).  Every GPU step runs under its own time limit: a step that
exceeds it ends the process (SIGALRM), so nothing more is started on the device.  `profile` as third argument adds one call
of (a) and (c) each on a profiling handle (per-phase rwr_stats times) -- a run of its own, not to be mixed with the timings.
    python tools/restart_eval_time.py [config] [out.jsonl] [profile]        (one JSON line per case, appended)"""
import ctypes as C
import json
import os
import signal
import sys
import time
from contextlib import contextmanager

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from recommendersystems_amd import _lib, synth
from recommendersystems_amd.rwr_based import Graph

cfg = sys.argv[1] if len(sys.argv) > 1 else "C2"
out_path = sys.argv[2] if len(sys.argv) > 2 and sys.argv[2] != "-" else None
profile_run = len(sys.argv) > 3 and sys.argv[3] == "profile"
T, S, TOP, N_TEST = 10, 8, 100, 50
KS = (64, 256)
d = float(np.float32(0.15))
PD, PI, PL = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)


@contextmanager
def limit(seconds):
    """the GPU step inside must end within `seconds`, or the process is ended by the alarm's default action"""
    signal.alarm(seconds)
    try:
        yield
    finally:
        signal.alarm(0)


g = synth.config(cfg)
flat = {k: g[k] for k in ("node_id", "node_type", "rowptr", "dst", "etype", "w")}
lib = _lib.load()
with limit(240):
    G = Graph.from_flat(**flat)
    G.buildGraph()
n = G.size()
nnz = int(g["rowptr"][-1])
hub = int(np.argmax(np.bincount(g["dst"][g["etype"] != 0], minlength=n)))
is_item = g["node_type"] == 2
n_items = int(is_item.sum())
item_ids = np.asarray(g["node_id"], dtype=np.int64)[is_item]


def emit(**kw):
    rec = dict(config=cfg, n=n, nnz=nnz, n_items=n_items, T=T, library=lib.rwr_version().decode(), **kw)
    print(json.dumps(rec), flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as f:
            f.write(json.dumps(rec) + "\n")


def eval_call(H, K, ptr, idx, val, steps, tp, ti, hits, sp, ln):
    t = time.perf_counter()
    _lib.check(lib.rwr_recommend_restart_eval_batch(H._handle(), K, ptr.ctypes.data_as(PL), idx.ctypes.data_as(PI),
                                                    val.ctypes.data_as(PD), None, None, None, d, steps, 0, tp.ctypes.data_as(PL),
                                                    ti.ctypes.data_as(PL), hits.ctypes.data_as(PL), sp.ctypes.data_as(PD),
                                                    ln.ctypes.data_as(PL)))
    return time.perf_counter() - t


def ranked_call(H, K, ptr, idx, val, steps, top_n, ids, sc, cnt):
    t = time.perf_counter()
    _lib.check(lib.rwr_recommend_restart_batch(H._handle(), K, ptr.ctypes.data_as(PL), idx.ctypes.data_as(PI), val.ctypes.data_as(PD),
                                               None, None, None, d, steps, top_n, ids.ctypes.data_as(PL), sc.ctypes.data_as(PD),
                                               cnt.ctypes.data_as(PI)))
    return time.perf_counter() - t


def host_eval(K, ids, cnt, tests):
    """Experiment.cs:121-128 over the K whole lists: (nHits, sumPrecision, listLen), and the time it took"""
    hits, sp, ln = np.zeros(K, dtype=np.int64), np.zeros(K), np.zeros(K, dtype=np.int64)
    t = time.perf_counter()
    for k in range(K):
        c = int(cnt[k])
        pos = np.flatnonzero(np.isin(ids[k, :c], tests[k]))
        terms = np.arange(1, len(pos) + 1, dtype=np.float64) / (pos + 1).astype(np.float64)
        hits[k], ln[k] = len(pos), c
        sp[k] = np.cumsum(terms)[-1] if len(pos) else 0.0        # cumsum adds left to right
    return hits, sp, ln, time.perf_counter() - t


def phases(K, ptr, fi, fv, tp, ti):
    H = Graph.from_flat(**flat, profile=True)
    H.buildGraph()
    hits, sp, ln = np.zeros(K, dtype=np.int64), np.zeros(K), np.zeros(K, dtype=np.int64)
    ids, sc, cnt = np.zeros((K, TOP), dtype=np.int64), np.zeros((K, TOP)), np.zeros(K, dtype=np.int32)
    out = {}
    for name, call in (("eval", lambda: eval_call(H, K, ptr, fi, fv, T, tp, ti, hits, sp, ln)),
                       ("top100", lambda: ranked_call(H, K, ptr, fi, fv, T, TOP, ids, sc, cnt))):
        with limit(120):
            call()
            lib.rwr_reset_stats(H._handle())
            wall = call()
        st = H.stats()
        out[name] = dict(wall_ms=round(wall * 1e3, 2), **{k: round(st[k], 3) for k in ("spmm_ms", "chain_ms", "rank_ms", "iterate_wall_ms")})
    H.close()
    return out


ms = lambda xs: [round(x * 1e3, 2) for x in xs]
rng = np.random.default_rng(2024)
for K in KS:
    idx = np.stack([rng.choice(n, S, replace=False) for _ in range(K)]).astype(np.int32)
    if hub not in idx[1]:
        idx[1, 0] = hub
    val = np.full((K, S), 1.0 / S)
    ptr = np.arange(0, (K + 1) * S, S, dtype=np.int64)
    fi, fv = np.ascontiguousarray(idx.reshape(-1)), np.ascontiguousarray(val.reshape(-1))
    tests = [rng.choice(item_ids, N_TEST, replace=False) for _ in range(K)]
    tp = np.arange(0, (K + 1) * N_TEST, N_TEST, dtype=np.int64)
    ti = np.ascontiguousarray(np.concatenate(tests))
    if profile_run:
        emit(case="restart_eval_phases", K=K, support=S, test_ids=N_TEST, phases=phases(K, ptr, fi, fv, tp, ti))
        continue
    hits, sp, ln = np.zeros(K, dtype=np.int64), np.zeros(K), np.zeros(K, dtype=np.int64)
    ids100, sc100, cnt100 = np.zeros((K, TOP), dtype=np.int64), np.zeros((K, TOP)), np.zeros(K, dtype=np.int32)
    ids, sc, cnt = np.ones((K, n_items), dtype=np.int64), np.ones((K, n_items)), np.zeros(K, dtype=np.int32)   # touched once
    with limit(180):                                         # warm-up at the full K: workspaces, in_w, every end's scratch
        eval_call(G, K, ptr, fi, fv, 2, tp, ti, hits, sp, ln)
        ranked_call(G, K, ptr, fi, fv, 2, TOP, ids100, sc100, cnt100)
        ranked_call(G, K, ptr, fi, fv, 2, n_items, ids, sc, cnt)
    a, b, c = [], [], []
    for _ in range(3):
        with limit(60):
            a.append(eval_call(G, K, ptr, fi, fv, T, tp, ti, hits, sp, ln))
    for _ in range(3):
        with limit(120):
            b.append(ranked_call(G, K, ptr, fi, fv, T, n_items, ids, sc, cnt))
    for _ in range(3):
        with limit(60):
            c.append(ranked_call(G, K, ptr, fi, fv, T, TOP, ids100, sc100, cnt100))
    hh, hs, hl, host = host_eval(K, ids, cnt, tests)
    equal = bool((hh == hits).all() and (hl == ln).all() and (hs.view(np.uint64) == sp.view(np.uint64)).all())
    st = G.stats()
    emit(case="restart_eval", K=K, support=S, test_ids=N_TEST, tile_seeds=st["tile_seeds"], tile_group=st["tile_group"],
         eval_ms=ms(a), full_lists_ms=ms(b), host_eval_ms=round(host * 1e3, 2), top100_ms=ms(c),
         eval_best_ms=round(min(a) * 1e3, 2), full_lists_best_ms=round(min(b) * 1e3, 2), top100_best_ms=round(min(c) * 1e3, 2),
         full_plus_host_ms=round((min(b) + host) * 1e3, 2), speedup_over_full_plus_host=round((min(b) + host) / min(a), 2),
         eval_over_top100=round(min(a) / min(c), 3), hits_total=int(hits.sum()),
         d2h_bytes_eval=K * 24, d2h_bytes_full_lists=K * n_items * 16 + K * 4, results_equal=equal)
    assert equal, "the evaluating call's results are not the host evaluation of the whole lists"
G.close()
