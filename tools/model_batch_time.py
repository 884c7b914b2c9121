"""K personalised Models in one call (rwr_model_run_batch) against K sequential rwr_model_run calls, on a BASELINE-config
graph (default C2), K = 256 seeds, T = 10 -- the numbers of DESIGN §3.9.
  * batch: the C entry point into ONE K x n output buffer touched beforehand (no page faults inside the timed calls), on a
    handle warmed with the same K (no workspace grows inside them), best of 3.  Split two ways: a T = 0 call (seed upload,
    initial vectors, extraction of every column, D2H), the steps' share being DERIVED as batch - T=0 call; and a profiled
    call on a second handle: iterate (device time of the steps), extraction (the column-extraction kernels) and the rest of
    THAT call's wall time (D2H + host work);
  * Model.RunBatch as a Python caller sees it: a fresh K x n array per call, best of 3;
  * sequential: 32 rwr_model_run calls timed, EXTRAPOLATED to K;
  * threshold: one batch call with value = 1e-9 * n, with the spread of the per-seed iteration counts.
    python tools/model_batch_time.py [config] [out.jsonl]        (one JSON line per case)"""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from recommendersystems_amd import _lib, synth
from recommendersystems_amd.rwr_based import Graph, Model

cfg = sys.argv[1] if len(sys.argv) > 1 else "C2"
out_path = sys.argv[2] if len(sys.argv) > 2 else None
K, T, SAMPLE = 256, 10, 32
d = float(np.float32(0.15))
g = synth.config(cfg)
flat = {k: g[k] for k in ("node_id", "node_type", "rowptr", "dst", "etype", "w")}
seeds = synth.seeds_for(g["users"], K, 0, K).astype(np.int32)
lib = _lib.load()
lines = []


def emit(**kw):
    rec = dict(config=cfg, K=K, library=lib.rwr_version().decode(), **kw)
    lines.append(rec)
    print(json.dumps(rec), flush=True)


G = Graph.from_flat(**flat)
G.buildGraph()
n = G.size()
nnz = int(g["rowptr"][-1])
P = C.POINTER(C.c_double)
dst = np.ones((K, n))                                        # one output buffer, touched once: no page faults in the timed calls
its = np.zeros(K, dtype=np.int64)
sp = seeds.ctypes.data_as(C.POINTER(C.c_int32))


def call(H, steps):
    t = time.perf_counter()
    _lib.check(lib.rwr_model_run_batch(H._handle(), sp, K, d, _lib.RWR_RUN_ITERATIONS, float(steps), dst.ctypes.data_as(P),
                                       its.ctypes.data_as(C.POINTER(C.c_int64))))
    return time.perf_counter() - t


call(G, 2)                                                   # warm-up at the full K: workspaces, chain-scan cells
best = min(call(G, T) for _ in range(3))
out_only = min(call(G, 0) for _ in range(3))                 # T = 0: seed upload, initial vectors, extraction, D2H
fresh = float("inf")                                         # what a Model.RunBatch caller sees: a fresh K x n array per call
for _ in range(3):
    t = time.perf_counter()
    Model.RunBatch(G, d, seeds, T)
    fresh = min(fresh, time.perf_counter() - t)

out = np.empty(n)
it = C.c_int64(0)
_lib.check(lib.rwr_model_run(G._handle(), int(seeds[0]), d, _lib.RWR_RUN_ITERATIONS, float(T), out.ctypes.data_as(P), C.byref(it)))
t = time.perf_counter()
for s in seeds[:SAMPLE].tolist():
    _lib.check(lib.rwr_model_run(G._handle(), s, d, _lib.RWR_RUN_ITERATIONS, float(T), out.ctypes.data_as(P), C.byref(it)))
seq_sample = time.perf_counter() - t
seq = seq_sample * K / SAMPLE
G.close()

Gp = Graph.from_flat(**flat, profile=True)                   # the same call with HIP events around its phases
Gp.buildGraph()
call(Gp, 2)                                                  # the same warm-up: the timed calls allocate no workspace
prof_wall, st = float("inf"), None
for _ in range(3):
    Gp.reset_stats()
    w = call(Gp, T)
    if w < prof_wall:
        prof_wall, st = w, Gp.stats()
Gp.close()
rest = prof_wall * 1e3 - st["iterate_wall_ms"] - st["rank_ms"]   # of the same profiled call
emit(case="iterations", n=n, nnz=nnz, T=T, tile_seeds=st["tile_seeds"], tile_group=st["tile_group"],
     batch_ms=round(best * 1e3, 2), batch_seeds_per_s=round(K / best, 1),
     sequential_ms_extrapolated=round(seq * 1e3, 2), sequential_sample_calls=SAMPLE,
     sequential_ms_per_call=round(seq_sample / SAMPLE * 1e3, 3), speedup=round(seq / best, 2),
     t0_call_ms=round(out_only * 1e3, 2), t0_call_share=round(out_only / best, 3),
     steps_ms_derived=round((best - out_only) * 1e3, 2),
     profiled_call_ms=round(prof_wall * 1e3, 2), iterate_ms=round(st["iterate_wall_ms"], 2),
     extraction_ms=round(st["rank_ms"], 2),
     d2h_and_host_ms=round(rest, 2), d2h_and_host_share=round(rest / (prof_wall * 1e3), 3),
     output_bytes=K * n * 8, d2h_gb_per_s_if_all_rest=round(K * n * 8 / (rest * 1e6), 1),
     fresh_array_call_ms=round(fresh * 1e3, 2), fresh_array_speedup=round(seq / fresh, 2))
del dst

G = Graph.from_flat(**flat)
G.buildGraph()
Model.RunBatch(G, d, seeds, 2)
value = 1e-9 * n
t = time.perf_counter()
ranks, iters = Model.RunBatch(G, d, seeds, value)
wall = time.perf_counter() - t
G.close()
emit(case="threshold", n=n, nnz=nnz, threshold=value, batch_ms=round(wall * 1e3, 2),
     iters_min=int(iters.min()), iters_median=float(np.median(iters)), iters_max=int(iters.max()),
     iters_distinct=int(len(set(iters.tolist()))))

if out_path:
    with open(out_path, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")
