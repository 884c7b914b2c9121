"""Graphs and the host reference of tests/test_gpu_long_lists.py: a list is the rank row filtered by a host model
of the marks, ranked by np.lexsort over (node asc, id desc, score desc) and walked greedily under the cap.  No GPU here."""
import numpy as np

from tests import graphgen as gg

R = 4096                    # long_plan.h: LONG_RUN
SEL_MAX_K = 1024            # rank_keys.h
SEL_CAP = 3072
LONG_TOP_N_MAX = 65536      # include/rwr.h: RWR_LONG_TOP_N_MAX
D = float(np.float32(0.15))                                      # the entries take a float and widen it
LIKE_MASK = 1 << gg.EDGE_LIKE
_GRAPHS = {}


def graph(name):
    """big: 12 400 users (more than 3R + 1 candidates), 300 items, a few ETC nodes; same_id: the same with one id for all users"""
    if name not in _GRAPHS:
        g = gg.random_graph(71, n_users=12400, n_items=300, n_likes=30000, n_etc=10, n_friend=3000, n_mention=500, n_author=100)
        if name == "same_id":
            g = dict(g)
            g["node_id"] = g["node_id"].copy()
            g["node_id"][g["node_type"] == gg.NODE_USER] = 5
        elif name != "big":
            raise KeyError(name)
        _GRAPHS[name] = g
    return _GRAPHS[name]


def whole_list(g, row, seed, cand_type, edge_types, exclude_self, pool, deny):
    """the node indices of one seed's whole list, best first"""
    n = len(row)
    ok = np.ones(n, dtype=bool) if cand_type is None else (g["node_type"] == cand_type)
    ok = ok.copy()
    if pool is not None:
        inside = np.zeros(n, dtype=bool)
        inside[np.asarray(pool, dtype=np.int64)] = True
        ok &= inside
    lo, hi = int(g["rowptr"][seed]), int(g["rowptr"][seed + 1])
    ok[g["dst"][lo:hi][np.isin(g["etype"][lo:hi], list(edge_types))]] = False
    if exclude_self:
        ok[seed] = False
    if deny is not None:
        ok[np.asarray(deny, dtype=np.int64)] = False
    rows = np.flatnonzero(ok)
    return rows[np.lexsort((rows, -g["node_id"][rows], -row[rows]))]


def greedy(rows, group_of, m):
    """the walk from the top with a counter per label; a negative label is never capped"""
    seen, kept = {}, []
    for i in rows.tolist():
        lb = int(group_of[i])
        if lb < 0:
            kept.append(i)
        elif seen.get(lb, 0) < m:
            kept.append(i)
            seen[lb] = seen.get(lb, 0) + 1
    return np.array(kept, dtype=np.int64)


def as_arrays(g, rows, lists, top_n):
    """the lists cut at top_n in the entries' layout: cells behind a list's end hold 0 / +0.0 / -1"""
    K = len(lists)
    ids, sc = np.zeros((K, top_n), dtype=np.int64), np.zeros((K, top_n))
    cnt, nodes = np.zeros(K, dtype=np.int32), np.full((K, top_n), -1, dtype=np.int32)
    for k, L in enumerate(lists):
        L = L[:top_n]
        cnt[k] = len(L)
        ids[k, :len(L)], sc[k, :len(L)], nodes[k, :len(L)] = g["node_id"][L], rows[k][L], L
    return ids, sc, cnt, nodes
