"""Graphs and NumPy references for the audience entry (rwr_recommend_audience_batch), shared by the CPU and GPU tests.

forward(): the literal loop of Model.deliverRanks (Model.cs:76-101) -- sources in node order, a source's links in list order,
the restart share of every source added to the seed's row as it is met -- for many seeds at once: the seeds are the rows of a
matrix, so every seed's arithmetic is exactly the scalar loop's.  reverse(): the recurrence of the audience entry -- the
dangling column h, the restart masses rho, then S per target.  check_lists(): the comparison of a returned batch with the
forward values that is safe under a tolerance."""
from __future__ import annotations

import numpy as np

from tests import graphgen as gg


# ---- normalisation (Graph.cs:53-86): explicit links divided by their list-order sum, UNDEFINED links carry no weight ---------
def normalise(g):
    rp, et, w = g["rowptr"], g["etype"], g["w"]
    n = len(rp) - 1
    wn = np.zeros(len(w), dtype=np.float64)
    nd = np.zeros(n, dtype=bool)
    for i in range(n):
        s = 0.0
        for p in range(rp[i], rp[i + 1]):
            if et[p] != gg.EDGE_UNDEFINED:
                s += float(w[p])
                nd[i] = True
        for p in range(rp[i], rp[i + 1]):
            if et[p] != gg.EDGE_UNDEFINED:
                wn[p] = float(w[p]) / s
    return wn, nd


def tol_rel(g, T, d):
    """8 (T + 1) (n + L + 8) 2^-53 / d, L = max(largest in-degree, largest out-degree): the bound the header derives."""
    rp, dst = g["rowptr"], g["dst"]
    n = len(rp) - 1
    L = 0
    if len(dst):
        L = max(int(np.diff(rp).max()), int(np.bincount(dst, minlength=n).max()))
    return 8.0 * (T + 1) * (n + L + 8) * 2.0 ** -53 / d


def forward(g, wn, nd, seeds, T, d):
    """F[j, v] = x_T^(seeds[j])[v], Model.cs's loop literally, one row per seed."""
    rp, dst = g["rowptr"], g["dst"]
    n = len(rp) - 1
    seeds = np.asarray(seeds, dtype=np.int64)
    ar = np.arange(len(seeds))
    x = np.zeros((len(seeds), n))
    x[ar, seeds] = n                                              # Model.cs:42-49
    for _ in range(T):
        nx = np.zeros_like(x)
        for i in range(n):
            if nd[i]:
                rw = (1 - d) * x[:, i]                            # Model.cs:84
                for p in range(rp[i], rp[i + 1]):
                    if g["etype"][p] != gg.EDGE_UNDEFINED:        # (Graph.graph holds the explicit links only)
                        nx[:, dst[p]] += rw * wn[p]               # Model.cs:87
                nx[ar, seeds] += x[:, i] - rw                     # Model.cs:91
            else:
                nx[ar, seeds] += x[:, i]                          # Model.cs:96-97
        x = nx
    return x


def _back(g, wn, c1, G):
    """B(g)[i] = (1 - d) sum_e w_e g[dst_e], list order; G: (n,) or (n, K)."""
    rp, dst = g["rowptr"], g["dst"]
    out = np.zeros_like(G)
    for i in range(len(rp) - 1):
        acc = np.zeros_like(G[0])
        for p in range(rp[i], rp[i + 1]):
            if wn[p] != 0.0:
                acc = acc + wn[p] * G[dst[p]]
        out[i] = c1 * acc
    return out


def dangling_columns(g, wn, nd, T, d):
    """h[j] for j < max(T, 1): h_0 = dangling, h_{j+1} = B(h_j)."""
    h = [(~nd).astype(np.float64)]
    for _ in range(T - 1):
        h.append(_back(g, wn, 1 - d, h[-1]))
    return np.array(h)


def rho_table(n, h, T, d):
    """rho[k] = d n + (1 - d) delta_k, delta_k = n h_k + sum_{m < k} rho_m h_{k-1-m}: every product and sum rounded on its own, m
    ascending -- the order of audience_plan.h's aud_rho_node."""
    rho = np.zeros((T, h.shape[1]))
    nn = float(n)
    for k in range(T):
        delta = nn * h[k]
        for m in range(k):
            delta = delta + rho[m] * h[k - 1 - m]
        rho[k] = d * nn + (1 - d) * delta
    return rho


def reverse(g, wn, nd, targets, T, d):
    """S[s, k] ~ x_T^(s)[targets[k]] for every s."""
    n = len(g["rowptr"]) - 1
    rho = rho_table(n, dangling_columns(g, wn, nd, T, d), T, d)
    G = np.zeros((n, len(targets)))
    G[np.asarray(targets, dtype=np.int64), np.arange(len(targets))] = 1.0
    S = np.zeros_like(G)
    for j in range(T):
        S = S + rho[T - 1 - j][:, None] * G
        G = _back(g, wn, 1 - d, G)
    return S + float(n) * G


# ---- the comparison ---------------------------------------------------------------------------------------------------------
def excluded_rows(g, target, mask, exclude_self):
    """the sources of the raw links into `target` whose type has its bit in the mask, and the target itself on request"""
    rp, dst, et = g["rowptr"], g["dst"], g["etype"]
    out = set()
    if mask:
        hit = (dst == target) & (((mask >> et.astype(np.int64)) & 1) == 1) & (et < 8)
        src = np.searchsorted(rp, np.nonzero(hit)[0], side="right") - 1
        out.update(int(s) for s in src)
    if exclude_self:
        out.add(int(target))
    return out


def candidates(g, cand_type):
    t = g["node_type"]
    return np.arange(len(t)) if cand_type is None or cand_type < 0 else np.nonzero(t == cand_type)[0]


def check_list(g, fcol, ids, scores, nodes, count, *, target, cand_type, mask, exclude_self, top_n, tol):
    """One returned list against fcol[s] = the forward score of `target` from seed s.  Holds when: every returned score is
    within tol of its forward value (+0.0 exactly where that is +0.0); the list is sorted by its own (score desc, id desc,
    index asc); every candidate left out has a forward score <= the last returned score * (1 + tol); excluded nodes are
    absent; count == min(top_n, candidates).  Returns the largest relative error seen."""
    node_id = g["node_id"]
    excl = excluded_rows(g, target, mask, exclude_self)
    cands = [int(c) for c in candidates(g, cand_type) if int(c) not in excl]
    assert count == min(top_n, len(cands)), (count, top_n, len(cands))
    got = [int(x) for x in nodes[:count]]
    assert len(set(got)) == count and set(got) <= set(cands), "a returned node is excluded, of another type, or listed twice"
    assert (nodes[count:] == -1).all()
    worst = 0.0
    for q, s in enumerate(got):
        assert ids[q] == node_id[s]
        f, v = float(fcol[s]), float(scores[q])
        if f == 0.0:
            assert v == 0.0 and not np.signbit(v), (s, v)
        else:
            err = abs(v - f) / f
            worst = max(worst, err)
            assert err <= tol, (s, v, f, err, tol)
    keys = [(-float(scores[q]), -int(ids[q]), got[q]) for q in range(count)]
    assert keys == sorted(keys), "the list is not sorted by (score desc, id desc, index asc)"
    if count and count < len(cands):
        last = float(scores[count - 1])
        rest = np.array(sorted(set(cands) - set(got)), dtype=np.int64)
        assert (fcol[rest] <= last * (1 + tol)).all(), "a candidate left out beats the last entry"
    return worst


# ---- graphs ----------------------------------------------------------------------------------------------------------------------
def from_lists(node_type, lists, node_id=None, seed=0):
    """lists[i]: [(target, edge type, raw weight), ...] in list order"""
    n = len(node_type)
    rng = np.random.default_rng(seed)
    if node_id is None:
        node_id = rng.permutation(np.arange(500, 500 + 3 * n, 3, dtype=np.int64))
    rowptr = np.zeros(n + 1, dtype=np.int64)
    dst, et, w = [], [], []
    for i in range(n):
        for (t, y, x) in lists[i]:
            dst.append(t); et.append(y); w.append(x)
        rowptr[i + 1] = len(dst)
    return dict(node_id=np.asarray(node_id, dtype=np.int64), node_type=np.asarray(node_type, dtype=np.uint8), rowptr=rowptr,
                dst=np.array(dst, dtype=np.int32), etype=np.array(et, dtype=np.uint8), w=np.array(w, dtype=np.float64))


def degree_graph(degs, seed, *, n_items=None, weighted=True, p_undefined=0.1, back_every=3):
    """Users 0 .. len(degs) - 1 with exactly degs[u] out-links (LIKE, to distinct items, some relabelled UNDEFINED inside the
    list), then the items; every back_every-th item links back to a user, the others are dangling.  The degrees are the
    point: 0, 1, 4, 5, 63, 64, 65 and the long-row split's edges."""
    rng = np.random.default_rng(seed)
    nu = len(degs)
    ni = n_items if n_items is not None else max(max(degs) + 3, 8)
    node_type = [gg.NODE_USER] * nu + [gg.NODE_ITEM] * ni
    lists = [[] for _ in range(nu + ni)]
    for u, dg in enumerate(degs):
        items = rng.permutation(ni)[:dg]
        for q, it in enumerate(items):
            y = gg.EDGE_UNDEFINED if (dg > 1 and q > 0 and rng.random() < p_undefined) else gg.EDGE_LIKE
            lists[u].append((nu + int(it), y, float(rng.integers(1, 6)) if weighted else 1.0))
    for it in range(0, ni, back_every):
        u = int(rng.integers(0, nu))
        lists[nu + it].append((u, gg.EDGE_LIKE, 1.0))
        if it % 2 == 0:
            lists[nu + it].append((int(rng.integers(0, nu)), gg.EDGE_AUTHORSHIP, 2.0 if weighted else 1.0))
    return from_lists(node_type, lists, seed=seed)


def drop_dangling(g):
    """the same graph with one LIKE link from every node without explicit links to node 0: no dangling node at all"""
    rp, et = g["rowptr"], g["etype"]
    n = len(rp) - 1
    lists = []
    for i in range(n):
        L = [(int(g["dst"][p]), int(et[p]), float(g["w"][p])) for p in range(rp[i], rp[i + 1])]
        if not any(y != gg.EDGE_UNDEFINED for (_, y, _) in L):
            L.append((0 if i != 0 else 1, gg.EDGE_LIKE, 1.0))
        lists.append(L)
    return from_lists(g["node_type"], lists, node_id=g["node_id"])
