"""K Models with caller-set restart vectors in one call (rwr_model_run_restart_batch) against the K sequential
rwr_model_run_restart calls it replaces, on a BASELINE-config graph (default C2), T = 10, d = 0.15f -- the numbers of
DESIGN §3.10.  K in {16, 64, 256} vectors of |S| in {1, 8, 64} random support rows each (the hub row in one of them), every
vector from the global constructor's rank.
  * batch: the C entry point into ONE K x n output buffer touched beforehand (no page faults inside the timed calls), on a
    handle warmed with the same batch (no workspace grows inside them), best of 3; the same batch at T = 0 (upload, initial
    ranks, extraction of every column, D2H), the steps' share being DERIVED as batch - T=0 call;
  * sequential: 8 rwr_model_run_restart calls timed (dense vectors built beforehand), EXTRAPOLATED to K;
  * the batch's rows of those 8 vectors must be bitwise the sequential calls' rows.
One more line, `link_only`: the K = 64 batch with empty supports (the weighted link-only SpMM steps alone, no chain) next to
rwr_model_run_batch at the same K (the value-free SpMM steps with their seed-row scans) -- what the SpMM costs beside the chains.
    python tools/restart_batch_time.py [config] [out.jsonl]        (one JSON line per case, appended)"""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from recommendersystems_amd import _lib, synth
from recommendersystems_amd.rwr_based import Graph

cfg = sys.argv[1] if len(sys.argv) > 1 else "C2"
out_path = sys.argv[2] if len(sys.argv) > 2 else None
T, SAMPLE = 10, 8
KS, SS = (16, 64, 256), (1, 8, 64)
d = float(np.float32(0.15))
g = synth.config(cfg)
flat = {k: g[k] for k in ("node_id", "node_type", "rowptr", "dst", "etype", "w")}
lib = _lib.load()
G = Graph.from_flat(**flat)
G.buildGraph()
n = G.size()
nnz = int(g["rowptr"][-1])
hub = int(np.argmax(np.bincount(g["dst"][g["etype"] != 0], minlength=n)))
PD, PI, PL = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
dst = np.ones((max(KS), n))                                  # one output buffer, touched once: no page faults in the timed calls
its = np.zeros(max(KS), dtype=np.int64)
ITER = _lib.RWR_RUN_ITERATIONS


def emit(**kw):
    rec = dict(config=cfg, n=n, nnz=nnz, T=T, library=lib.rwr_version().decode(), **kw)
    print(json.dumps(rec), flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as f:
            f.write(json.dumps(rec) + "\n")


def batch_call(K, ptr, idx, val, steps):
    t = time.perf_counter()
    _lib.check(lib.rwr_model_run_restart_batch(G._handle(), K, ptr.ctypes.data_as(PL), idx.ctypes.data_as(PI), val.ctypes.data_as(PD),
                                               None, d, ITER, float(steps), dst.ctypes.data_as(PD), its.ctypes.data_as(PL)))
    return time.perf_counter() - t


rng = np.random.default_rng(2024)
x0 = np.ones(n)
one = np.empty(n)
it1 = C.c_int64(0)
for K in KS:
    for S in SS:
        idx = np.stack([rng.choice(n, S, replace=False) for _ in range(K)]).astype(np.int32)
        if hub not in idx[1]:
            idx[1, 0] = hub                                  # the hub row in one of the timed sample's vectors
        val = np.full((K, S), 1.0 / S)
        ptr = np.arange(0, (K + 1) * S, S, dtype=np.int64)
        fi, fv = np.ascontiguousarray(idx.reshape(-1)), np.ascontiguousarray(val.reshape(-1))
        batch_call(K, ptr, fi, fv, 2)                        # warm-up at the full K: workspaces, in_w
        best = min(batch_call(K, ptr, fi, fv, T) for _ in range(3))
        rows = dst[:SAMPLE].copy()
        t0 = min(batch_call(K, ptr, fi, fv, 0) for _ in range(3))
        vs = []
        for k in range(SAMPLE):
            v = np.zeros(n)
            v[idx[k]] = val[k]
            vs.append(v)
        _lib.check(lib.rwr_model_run_restart(G._handle(), vs[0].ctypes.data_as(PD), x0.ctypes.data_as(PD), d, ITER, 2.0,
                                             one.ctypes.data_as(PD), C.byref(it1)))   # warm-up (the single call's buffers)
        seq_sample, bitwise = 0.0, True
        for k in range(SAMPLE):
            t = time.perf_counter()
            _lib.check(lib.rwr_model_run_restart(G._handle(), vs[k].ctypes.data_as(PD), x0.ctypes.data_as(PD), d, ITER, float(T),
                                                 one.ctypes.data_as(PD), C.byref(it1)))
            seq_sample += time.perf_counter() - t
            bitwise = bitwise and bool((one.view(np.uint64) == rows[k].view(np.uint64)).all())
        seq = seq_sample * K / SAMPLE
        st = G.stats()
        emit(case="restart_batch", K=K, support=S, chains=K * S, tile_seeds=st["tile_seeds"], tile_group=st["tile_group"],
             batch_ms=round(best * 1e3, 2), batch_step_ms_derived=round((best - t0) / T * 1e3, 3), t0_call_ms=round(t0 * 1e3, 2),
             sequential_ms_extrapolated=round(seq * 1e3, 2), sequential_sample_calls=SAMPLE,
             sequential_ms_per_call=round(seq_sample / SAMPLE * 1e3, 3), speedup=round(seq / best, 2),
             sample_rows_bitwise=bitwise)
        assert bitwise, "the batch's rows are not bitwise the sequential calls' rows"

K = 64
ptr0 = np.zeros(K + 1, dtype=np.int64)
e_i, e_v = np.zeros(1, dtype=np.int32), np.zeros(1)
batch_call(K, ptr0, e_i, e_v, 2)
lo = min(batch_call(K, ptr0, e_i, e_v, T) for _ in range(3))
lo0 = min(batch_call(K, ptr0, e_i, e_v, 0) for _ in range(3))
seeds = synth.seeds_for(g["users"], K, 0, K).astype(np.int32)


def seed_call(steps):
    t = time.perf_counter()
    _lib.check(lib.rwr_model_run_batch(G._handle(), seeds.ctypes.data_as(PI), K, d, ITER, float(steps), dst.ctypes.data_as(PD),
                                       its.ctypes.data_as(PL)))
    return time.perf_counter() - t


seed_call(2)
sb = min(seed_call(T) for _ in range(3))
sb0 = min(seed_call(0) for _ in range(3))
emit(case="link_only", K=K, support=0, uniform_graph=bool(G.stats()["uniform"]),
     weighted_link_only_step_ms=round((lo - lo0) / T * 1e3, 3), link_only_batch_ms=round(lo * 1e3, 2),
     seed_batch_step_ms=round((sb - sb0) / T * 1e3, 3), seed_batch_ms=round(sb * 1e3, 2))
G.close()
