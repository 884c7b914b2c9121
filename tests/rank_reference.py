"""Exact reference of the ranking stage (Recommender.cs:20-38) over a given rank vector, in plain NumPy.

The candidates are the ITEM nodes that the seed does not LIKE: the exclusion list is the seed's RAW out-links of type
LIKE (:20-24, `Contains` semantics, so duplicates change nothing and a seed that is itself an ITEM stays a candidate
unless it LIKEs itself).  They are ordered by score descending, then id descending (:35-38, double.CompareTo and
long.CompareTo).  Scores are returned as the rank vector holds them, bit patterns untouched.

Used by the tests as the yardstick of every top-k path of the HIP library (rank.hip, sort.hip, small.hip); its own
agreement with the oracle is pinned by tests/test_rank_reference.py.
"""
from __future__ import annotations

import numpy as np

NODE_ITEM = 2
EDGE_LIKE = 1


def candidate_rows(node_type, rowptr, dst, etype, seed: int) -> np.ndarray:
    """Rows of the ranking's candidates in ascending row order: ITEM nodes minus the seed's raw LIKE targets."""
    node_type = np.asarray(node_type)
    lo, hi = int(rowptr[seed]), int(rowptr[seed + 1])
    liked = np.asarray(dst[lo:hi], dtype=np.int64)[np.asarray(etype[lo:hi]) == EDGE_LIKE]
    cand = node_type == NODE_ITEM
    cand[liked] = False
    return np.flatnonzero(cand)


def reference_ranking(rank, node_id, node_type, rowptr, dst, etype, seed: int, top_n: int = 0):
    """(ids, scores, count) of Recommendation(seed, ..., topN) for the rank vector `rank`; top_n <= 0: the whole list
    (Recommender.cs:42-51 never truncates then)."""
    rank = np.asarray(rank, dtype=np.float64)
    node_id = np.asarray(node_id, dtype=np.int64)
    rows = candidate_rows(node_type, rowptr, dst, etype, seed)
    s = rank[rows]
    ids = node_id[rows]
    # np.lexsort: ascending, stable, last key primary.  (score, id) pairs are unique (ids of items are unique), so the
    # reversed ascending order is exactly score descending, then id descending; -0.0 and +0.0 compare equal, as in C#
    order = np.lexsort((ids, s))[::-1]
    if top_n > 0:
        order = order[:top_n]
    return ids[order].copy(), s[order].copy(), int(order.shape[0])


def reference_batch(ranks, node_id, node_type, rowptr, dst, etype, seeds, top_n: int):
    """reference_ranking for every row of `ranks` (K x n), packed as rwr_recommend_batch returns it: ids / scores
    K x top_n (zero past each row's count) and counts."""
    K = len(seeds)
    ids = np.zeros((K, top_n), dtype=np.int64)
    sc = np.zeros((K, top_n), dtype=np.float64)
    cnt = np.zeros(K, dtype=np.int32)
    for k, seed in enumerate(seeds):
        i, s, c = reference_ranking(ranks[k], node_id, node_type, rowptr, dst, etype, int(seed), top_n)
        ids[k, :c] = i
        sc[k, :c] = s
        cnt[k] = c
    return ids, sc, cnt
