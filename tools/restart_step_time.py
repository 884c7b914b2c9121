"""Per-step time of a Model with a caller-set restart vector (rwr_model_run_restart) on a BASELINE-config graph, for
|S| = 1, 8, 256 non-zero restart entries (bitwise class: one k_restart_fold chain per support row beside the link-only
SpMV) and a dense vector (tolerance class), next to the seed path's step (rwr_model_run, seed >= 0) for comparison.
A step is timed as the difference of a 12-step and a 2-step run over 10 steps (upload, read-back and set-up cancel).
    python tools/restart_step_time.py [config] [out.jsonl]        (default C2; one JSON line per case)"""
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
g = synth.config(cfg)
U = g["users"]
G = Graph.from_flat(**{k: g[k] for k in ("node_id", "node_type", "rowptr", "dst", "etype", "w")})
G.buildGraph()
lib = _lib.load()
n = G.size()
nnz = int(g["rowptr"][-1])
d = 0.15
seed = int(synth.seeds_for(U, 256, 0, 1)[0])
x0 = np.zeros(n)
x0[seed] = float(n)
out = np.empty(n)
P = C.POINTER(C.c_double)
it = C.c_int64(0)


def run_restart(v, T):
    _lib.check(lib.rwr_model_run_restart(G._handle(), v.ctypes.data_as(P), x0.ctypes.data_as(P), d, _lib.RWR_RUN_ITERATIONS,
                                         float(T), out.ctypes.data_as(P), C.byref(it)))


def run_seed(_, T):
    _lib.check(lib.rwr_model_run(G._handle(), seed, d, _lib.RWR_RUN_ITERATIONS, float(T), out.ctypes.data_as(P), C.byref(it)))


def step_ms(fn, v, reps=3):
    fn(v, 2)                                              # warm-up (workspaces, in_w)
    best = {}
    for T in (2, 12):
        ts = []
        for _ in range(reps):
            t = time.perf_counter()
            fn(v, T)
            ts.append(time.perf_counter() - t)
        best[T] = min(ts)
    return (best[12] - best[2]) / 10 * 1e3


cases = []
for k in (1, 8, 256):
    v = np.zeros(n)
    v[synth.seeds_for(U, k, 0, k)] = 1.0 / k
    cases.append((f"restart_S{k}", run_restart, v))
cases.append(("restart_dense", run_restart, np.full(n, 1.0 / n)))
cases.append(("seed_path", run_seed, None))
lines = []
for name, fn, v in cases:
    ms = step_ms(fn, v)
    sup = int(np.count_nonzero(v)) if v is not None else 1
    rec = dict(config=cfg, n=n, nnz=nnz, case=name, support=sup, step_ms=round(ms, 4),
               parity="bitwise" if sup <= 256 else "tolerance", library=_lib.load().rwr_version().decode())
    print(json.dumps(rec), flush=True)
    lines.append(json.dumps(rec))
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
