#!/usr/bin/env python3
"""CPU study behind the size of the exact head of a batch's last step ("A smaller head").

Tiles are built the way recommend_batch builds them (upload_seed_slots: the live seeds, in-degree-descending, stable, dealt
round-robin over the tiles), so every tile holds some of the batch's heaviest seeds.  Per tile: x9 per seed from
oracle.c_oracle.FlatGraph.model_run (T - 1 steps), the value-free z, one more step for the item scores.  For every head size
H of the sweep, tau[s](H) = the top_n-th non-excluded score among the first H ITEM rows by in-degree (what k_sel_tau reads
after an exact ranking of those rows), and the rows the bound of rank_bound.h prunes under those thresholds.  From these:

  single stage, head H0:   head in-links | in-links of the body rows the bound keeps | worst seed's candidate count (rows
                           outside the head with score >= tau, liked items included)
  two stages, H0 < H1:     the head; rows [H0, H1) pruned with tau(H0), merged; rows [H1, n_items) pruned with tau(H1), which is
                           what the merged list's top_n-th score is: the merge is exact over [0, H1)

Cost model, in 256-byte row gathers per tile: head in-links + kept in-links + (in-links the bound pass walks) / 32, turned into
milliseconds with the committed trace's head (profiles/rank_prune_C4_kernel_stats_after.csv: 71 ms for the in-links of C4's
524 288-row head; pass --ms-per-mlink for another figure), plus 3.5 ms of fixed kernels per extra stage.

Asserted: no pruned row reaches any threshold it was pruned under.

    python tools/rank_head_study.py --config C4 --tiles 4 --out profiles/rank_head_study.json
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rank_prune_study import D, G, SLACK, T, TOP_N  # noqa: E402

SEL_SLOTS = 4096                                   # rank_keys.h
CAPACITY = SEL_SLOTS - TOP_N
STAGE_MS = 3.5                                     # k_sel_bound_table, _compact, _flags, the merge: per extra stage
H_MIN, H_MAX = 8192, 524288
MIDS = (2, 4, 8)


def deal_tiles(seeds, indeg, tile_seeds=G):
    """upload_seed_slots' rule: batch positions ordered by the seed's in-degree, highest first, stable; rank r goes to tile
    r % ntiles, slot r // ntiles.  Returns an (ntiles, tile_seeds) array of seeds, -1 in padded slots."""
    seeds = np.asarray(seeds)
    K = int(seeds.shape[0])
    ntiles = (K + tile_seeds - 1) // tile_seeds
    order = np.argsort(-np.asarray(indeg)[seeds].astype(np.int64), kind="stable")
    tiles = np.full((ntiles, tile_seeds), -1, dtype=np.int64)
    r = np.arange(K)
    tiles[r % ntiles, r // ntiles] = seeds[order]
    return tiles


def head_sizes(n_items):
    hs, h = [], H_MIN
    while h <= H_MAX * MIDS[-1]:
        if h < n_items:
            hs.append(h)
        h *= 2
    return hs


def study_tile(fg, g, seeds, order, threads):
    U, I = g["users"], g["items"]
    rowptr, dst = fg.rowptr, fg.dst
    outdeg = np.diff(rowptr)
    live = [int(s) for s in seeds if s >= 0]
    with ThreadPoolExecutor(max_workers=threads) as ex:
        xs = list(ex.map(lambda s: fg.model_run(D, seed=s, mode=0, value=float(T - 1))[0][:U].copy(), live))
    w_src = np.zeros(U)
    w_src[outdeg[:U] > 0] = 1.0 / outdeg[:U][outdeg[:U] > 0]
    item_ptr = rowptr[U:] - rowptr[U]                 # in-lists of the ITEM rows = their own (symmetric) lists
    src = dst[rowptr[U]:]
    indeg = np.diff(item_ptr)
    nz = indeg > 0
    starts = item_ptr[:-1][nz]

    def row_sums(v, dtype):
        out = np.zeros(I, dtype=dtype)
        out[nz] = np.add.reduceat(v[src].astype(dtype, copy=False), starts)
        return out

    pos = np.empty(I, dtype=np.int64)                 # position of an ITEM row in the in-degree order
    pos[order] = np.arange(I)
    deg_ord = indeg[order].astype(np.int64)
    links_cum = np.concatenate([[0], np.cumsum(deg_ord)])
    Hs = head_sizes(I)
    zs, sc_ord, liked_pos = [], [], []
    for s, x in zip(live, xs):
        z = ((1.0 - D) * x) * w_src
        zs.append(z)
        sc_ord.append(row_sums(z, np.float64)[order])
        liked_pos.append(pos[dst[rowptr[s]:rowptr[s + 1]] - U])
    del xs

    # per head size: thresholds, the kept in-links as a running sum along the order, candidates per seed up to every boundary
    bounds = Hs + [I]
    per_h = {}
    for H in Hs:
        taus = []
        for sc, lp in zip(sc_ord, liked_pos):
            hs = sc[:H].copy()
            hs[lp[lp < H]] = -1.0
            taus.append(float(np.partition(hs, H - TOP_N)[H - TOP_N]) if H >= TOP_N else 0.0)
        no_prune = any(t <= 0.0 for t in taus)
        m = np.zeros(U, dtype=np.float64)
        for z, t in zip(zs, taus):
            if t > 0.0:
                np.maximum(m, z / t, out=m)
        m32 = np.nextafter(m.astype(np.float32), np.float32(np.inf))
        prunable = ((row_sums(m32, np.float32) * SLACK < np.float32(1.0)) & (not no_prune))[order]
        cand = np.zeros((len(live), len(bounds)), dtype=np.int64)   # rows at positions [H, b) with score >= tau
        for i, (sc, t) in enumerate(zip(sc_ord, taus)):
            reach = sc >= t
            assert not np.any(prunable[H:] & reach[H:]), "a pruned row reaches tau: the bound is wrong"
            c = np.concatenate([[0], np.cumsum(reach)])
            cand[i] = [int(c[b] - c[H]) if b >= H else 0 for b in bounds]
        kept_cum = np.concatenate([[0], np.cumsum(deg_ord * ~prunable)])
        per_h[H] = {"taus": taus, "no_prune": no_prune, "kept_cum": kept_cum, "cand": cand}

    def stage(H, a, b):
        """rows at positions [a, b) pruned under tau(H): kept in-links, walked in-links, worst seed's candidates"""
        p = per_h[H]
        c = p["cand"][:, bounds.index(b)] - p["cand"][:, bounds.index(a)]
        return int(p["kept_cum"][b] - p["kept_cum"][a]), int(links_cum[b] - links_cum[a]), int(c.max())

    res = {"seeds": live, "max_likes": int(outdeg[live].max()), "single": {}, "staged": {}}
    for H0 in [h for h in Hs if h <= H_MAX]:
        kept, walked, worst = stage(H0, H0, I)
        res["single"][str(H0)] = {"head_links": int(links_cum[H0]), "kept_links": kept, "walked_links": walked,
                                  "worst_candidates": worst, "tau_min": min(per_h[H0]["taus"])}
        for f in MIDS:
            H1 = H0 * f
            if H1 not in per_h:
                continue
            k2, w2, c2 = stage(H0, H0, H1)
            k3, w3, c3 = stage(H1, H1, I)
            res["staged"][f"{H0},{H1}"] = {"head_links": int(links_cum[H0]), "kept_links": [k2, k3], "walked_links": [w2, w3],
                                           "worst_candidates": [c2, c3]}
    return res


def gathers(head_links, kept, walked):
    return head_links + kept + walked / 32.0


def summarise(tiles, ms_per_mlink):
    """worst tile's modelled cost and the worst seed's candidate count, per setting"""
    out = {"single": {}, "staged": {}}
    for key in next(iter(tiles.values()))["single"]:
        rs = [t["single"][key] for t in tiles.values()]
        gs = max(gathers(r["head_links"], r["kept_links"], r["walked_links"]) for r in rs)
        out["single"][key] = {"gathers_per_tile": round(gs), "model_ms": round(gs * 1e-6 * ms_per_mlink, 2),
                              "kept_links_max": max(r["kept_links"] for r in rs),
                              "worst_candidates": max(r["worst_candidates"] for r in rs)}
    for key in next(iter(tiles.values()))["staged"]:
        rs = [t["staged"][key] for t in tiles.values()]
        gs = max(gathers(r["head_links"], sum(r["kept_links"]), sum(r["walked_links"])) for r in rs)
        out["staged"][key] = {"gathers_per_tile": round(gs), "model_ms": round(gs * 1e-6 * ms_per_mlink + STAGE_MS, 2),
                              "kept_links_max": [max(r["kept_links"][i] for r in rs) for i in (0, 1)],
                              "worst_candidates": [max(r["worst_candidates"][i] for r in rs) for i in (0, 1)]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C4")
    ap.add_argument("--tiles", type=int, default=4, help="tiles studied: 0 .. tiles-1 of the dealt batch (the heaviest seeds lead them)")
    ap.add_argument("--threads", type=int, default=max(1, min(8, os.cpu_count() or 1)))
    ap.add_argument("--ms-per-mlink", type=float, default=0.0,
                    help="milliseconds per million row gathers per tile (0: 71 ms over the in-links of C4's 524 288-row head)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    t0 = time.time()
    from oracle.c_oracle import FlatGraph
    from recommendersystems_amd import synth
    g = synth.config(args.config)
    fg = FlatGraph(g["node_id"], g["node_type"], g["rowptr"], g["dst"], g["etype"], g["w"])
    U, I, K = g["users"], g["items"], g["seeds_per_gpu"]
    outdeg = np.diff(fg.rowptr)
    all_seeds = synth.seeds_for(U, K, 0, K)
    live = all_seeds[outdeg[all_seeds] > 0]           # dangling seeds are answered without iterating and take no slot
    tiles = deal_tiles(live, outdeg)                  # (a like-graph is symmetric: a user's in-degree is its out-degree)
    order = np.argsort(-outdeg[U:], kind="stable")    # ITEM rows by in-degree, highest first
    out = {"config": args.config, "users": U, "items": I, "likes": g["likes"], "T": T, "top_n": TOP_N, "G": G, "d": D,
           "capacity": CAPACITY, "batch_tiles": int(tiles.shape[0]), "tiles": {}}
    for t in range(min(args.tiles, tiles.shape[0])):
        out["tiles"][str(t)] = study_tile(fg, g, tiles[t], order, args.threads)
        print(json.dumps({t: out["tiles"][str(t)]["single"]}), flush=True)
    ms = args.ms_per_mlink
    if ms <= 0.0:
        # C4's 524 288-row head: 71 ms (committed trace); its in-links, from C4's own in-degrees when that is the graph studied
        ms = 71.0 / (out["tiles"]["0"]["single"]["524288"]["head_links"] * 1e-6) if args.config == "C4" else 0.0
    if ms <= 0.0:
        raise SystemExit("--ms-per-mlink is needed for a graph other than C4 (take C4's summary.ms_per_mlink)")
    out["ms_per_mlink"] = ms
    out["summary"] = summarise(out["tiles"], ms)
    out["seconds"] = round(time.time() - t0, 1)
    print(json.dumps(out["summary"], indent=1))
    if args.out:                                      # one file, one entry per graph
        both = {}
        if os.path.exists(args.out):
            with open(args.out) as f:
                both = json.load(f)
        both[args.config] = out
        with open(args.out, "w") as f:
            json.dump(both, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
