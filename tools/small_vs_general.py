import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from recommendersystems_amd import synth
from recommendersystems_amd.rwr_based import Graph, Recommender
for (U, I, E) in ((300, 1500, 5000), (600, 2500, 12000), (1000, 3000, 27500), (1200, 3500, 40000), (1500, 4000, 48000)):
    g = synth.bipartite(9, U, I, E)
    flat = {k: g[k] for k in ("node_id", "node_type", "rowptr", "dst", "etype", "w")}
    G = Graph.from_flat(**flat); G.buildGraph()
    rec = Recommender(G)
    rec.RecommendationArrays(0, 0.15, 10)
    N = 30
    t = time.perf_counter()
    for _ in range(N):
        rec.RecommendationArrays(0, 0.15, 10)
    print(f"RWR_SMALL={os.environ.get('RWR_SMALL','1')} n={U+I} nnz={len(g['dst'])}: call {(time.perf_counter()-t)/N*1e6:.0f} us", flush=True)
