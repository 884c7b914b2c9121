"""Host-side mirror of the reference's public surface ``namespace Recommenders.RWRBased``
(Recommenders/RWRBased/{Graph,Model,Recommender}.cs) over the librwr C-ABI.

Same names, argument meaning and error behaviour as the C# types, so the parity tests read
like the reference's caller (TweetRecommender/Experiment.cs:104-109).  The reference is
C#, which cannot be built in this image; the C# shim that a .NET host would use is under
csharp/ and P/Invokes exactly the functions used here.

All arithmetic happens in hand-written HIP kernels on the GPU; this module only flattens the
reference's containers into the SoA layout of include/rwr.h and wraps results.
"""
from __future__ import annotations

import ctypes as C
import enum
import itertools
from typing import Dict, List, Optional, Tuple

import numpy as np

from . import _lib


class NodeType(enum.IntEnum):
    """Recommender.cs:4."""
    UNDEFINED = 0
    USER = 1
    ITEM = 2
    ETC = 3


class EdgeType(enum.IntEnum):
    """Recommender.cs:5."""
    UNDEFINED = 0
    LIKE = 1
    FRIENDSHIP = 2
    FOLLOW = 3
    MENTION = 4
    AUTHORSHIP = 5
    PURCHASE = 6
    ETC = 7


class Node:
    """struct Node (Graph.cs:4-17)."""
    __slots__ = ("id", "type")

    def __init__(self, id: int, type: NodeType = NodeType.UNDEFINED):
        self.id = int(id)
        self.type = NodeType(type)


class ForwardLink:
    """struct ForwardLink (Graph.cs:19-35); fields are public and mutable, as the harness
    relies on (DataLoader.cs:66,424; Experiment.cs:90-97)."""
    __slots__ = ("targetNode", "type", "weight")

    def __init__(self, targetNode: int, type=EdgeType.UNDEFINED, weight: Optional[float] = None):
        # ForwardLink(int, double) and ForwardLink(int, EdgeType, double)
        if weight is None:
            type, weight = EdgeType.UNDEFINED, type
        self.targetNode = int(targetNode)
        self.type = EdgeType(type)
        self.weight = float(weight)


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def _pack_tests(testSets, K):
    """K collections of test ids in the caller's order as CSR, and the result arrays of a positions entry: one position and
    one score per entry (at least one element behind each pointer), one list length per batch position"""
    tests = [np.asarray(list(t), dtype=np.int64).reshape(-1) for t in testSets]
    if len(tests) != K:
        raise ValueError(f"testSets must hold {K} id collections")
    tp = np.zeros(K + 1, dtype=np.int64)
    tp[1:] = np.cumsum([len(t) for t in tests])
    ti = np.ascontiguousarray(np.concatenate(tests) if K else np.zeros(0, dtype=np.int64), dtype=np.int64)
    total = max(int(tp[K]), 1)
    return tp, ti, np.full(total, -1, dtype=np.int64), np.zeros(total, dtype=np.float64), np.zeros(K, dtype=np.int64)


def _pack_filter(pool, deny, K):
    """The pool and the K deny lists of a filtered entry as it takes them: (pool_count, pool_idx, deny_ptr, deny_idx).
    pool None: count -1 and no array, an empty pool: count 0; deny None: no arrays, else CSR over the batch positions (at
    least one element behind each pointer that is passed)"""
    def idx32(a):                                                # (an array is taken as it is: no trip through a Python list)
        a = a if isinstance(a, np.ndarray) else np.asarray(list(a), dtype=np.int64)
        if a.dtype != np.int32 and a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
            raise OverflowError("a node index does not fit int32")
        return np.ascontiguousarray(a, dtype=np.int32).reshape(-1)

    pc, pi, dp, di = -1, None, None, None
    if pool is not None:
        flat = idx32(pool)
        pc = int(flat.shape[0])
        pi = flat if pc else np.zeros(1, dtype=np.int32)
    if deny is not None:
        sets = [idx32(e) for e in deny]
        if len(sets) != K:
            raise ValueError(f"deny must hold {K} node lists")
        dp = np.zeros(K + 1, dtype=np.int64)
        dp[1:] = np.cumsum([len(e) for e in sets])
        di = np.ascontiguousarray(np.concatenate(sets + [np.zeros(0, dtype=np.int32)]), dtype=np.int32)
        if di.shape[0] == 0:
            di = np.zeros(1, dtype=np.int32)
    return pc, pi, dp, di


def _pack_groups(groupOf):
    """The labels of a capped entry as it takes them: an int32 array of one label per node (an array is taken as it is, no
    trip through a Python list), or None for no cap"""
    if groupOf is None:
        return None
    a = groupOf if isinstance(groupOf, np.ndarray) else np.asarray(list(groupOf), dtype=np.int64)
    if a.dtype != np.int32 and a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
        raise OverflowError("a group label does not fit int32")
    a = np.ascontiguousarray(a, dtype=np.int32).reshape(-1)
    return a if a.size else np.zeros(1, dtype=np.int32)


def _split_tests(tp, flat):
    return [flat[int(tp[k]):int(tp[k + 1])].copy() for k in range(len(tp) - 1)]


def _grown_lists(old_flat, new_flat):
    """The links by which the lists of ``new_flat`` exceed those of ``old_flat`` (both as ``Graph._flatten`` returns them):
    ``(src, dst, etype, w)`` of the appended links, row by row in list order, when the node arrays are equal and every old
    list is a bitwise prefix of the new one (weights compared as uint64); ``None`` otherwise.  No change gives empty arrays."""
    o_id, o_type, o_rp, o_dst, o_et, o_w = old_flat
    n_id, n_type, n_rp, n_dst, n_et, n_w = new_flat
    if o_id.shape != n_id.shape or not ((o_id == n_id).all() and (o_type == n_type).all()):
        return None
    o_len, n_len = np.diff(o_rp), np.diff(n_rp)
    if (n_len < o_len).any():
        return None
    n = int(o_id.shape[0])
    rows = np.arange(n, dtype=np.int64)
    # where the old link at flat position e sits in the new lists: same row, same place in the row
    kept = np.arange(int(o_rp[n]), dtype=np.int64) + np.repeat(n_rp[:-1] - o_rp[:-1], o_len)
    if not ((n_dst[kept] == o_dst).all() and (n_et[kept] == o_et).all()
            and (n_w[kept].view(np.uint64) == o_w.view(np.uint64)).all()):
        return None
    added = np.ones(int(n_rp[n]), dtype=bool)
    added[kept] = False
    src = np.repeat(rows, n_len - o_len).astype(np.int32)
    return src, n_dst[added], n_et[added], n_w[added]


def _extended_flat(flat, node_id, node_type):
    """``flat`` with the nodes (node_id, node_type) behind its last node, each with an empty list: what
    rwr_graph_append_nodes does to the node arrays and the row pointers.  The link arrays are shared, not copied."""
    o_id, o_type, o_rp, o_dst, o_et, o_w = flat
    k = int(node_id.shape[0])
    return (np.concatenate([o_id, node_id]), np.concatenate([o_type, node_type]),
            np.concatenate([o_rp, np.full(k, o_rp[-1], dtype=np.int64)]), o_dst, o_et, o_w)


def _grown_nodes(old_flat, new_flat):
    """``(n_old, (src, dst, etype, w))`` when ``new_flat`` is ``old_flat`` with nodes added behind its last one (the old
    nodes unchanged) and every old list a bitwise prefix of the new one -- the links as ``_grown_lists`` returns them, with
    the new nodes' lists starting empty; ``None`` otherwise, and when no node was added."""
    o_id, o_type = old_flat[0], old_flat[1]
    n_id, n_type = new_flat[0], new_flat[1]
    n_old = int(o_id.shape[0])
    if n_id.shape[0] <= n_old or not ((n_id[:n_old] == o_id).all() and (n_type[:n_old] == o_type).all()):
        return None
    grown = _grown_lists(_extended_flat(old_flat, n_id[n_old:], n_type[n_old:]), new_flat)
    return None if grown is None else (n_old, grown)


def _merged_flat(flat, src, dst, etype, w, pos):
    """``flat`` (as ``Graph._flatten`` returns it) with the links (src, dst, etype, w) at the positions ``pos`` that
    rwr_graph_append_links gave them: new arrays, the old links in their order in the places in between."""
    node_id, node_type, rowptr, o_dst, o_et, o_w = flat
    n = int(node_id.shape[0])
    m_new = int(rowptr[n]) + int(pos.shape[0])
    old = np.ones(m_new, dtype=bool)
    old[pos] = False
    out = []
    for o, a in ((o_dst, dst), (o_et, etype), (o_w, w)):
        x = np.empty(m_new, dtype=o.dtype)
        x[old] = o
        x[pos] = a
        out.append(x)
    new_rowptr = rowptr.copy()
    new_rowptr[1:] += np.cumsum(np.bincount(src, minlength=n).astype(np.int64))
    return (node_id, node_type, new_rowptr, out[0], out[1], out[2])


def _shrunk_lists(old_flat, new_flat):
    """The positions (in ``old_flat``'s flattened raw list, ascending) of the links by which the lists of ``old_flat`` exceed
    those of ``new_flat``: the node arrays are equal, no list is longer, every list of unchanged length is bitwise equal, and
    every shorter list is a subsequence of its old self by (target, type, weight bits).  ``None`` otherwise.  Where several
    old links could be the ones that left (copies of one link in one list), the earliest match is kept: any choice leaves
    the same lists.  No change gives an empty array."""
    o_id, o_type, o_rp, o_dst, o_et, o_w = old_flat
    n_id, n_type, n_rp, n_dst, n_et, n_w = new_flat
    if o_id.shape != n_id.shape or not ((o_id == n_id).all() and (o_type == n_type).all()):
        return None
    o_len, n_len = np.diff(o_rp), np.diff(n_rp)
    if (n_len > o_len).any():
        return None
    o_wb, n_wb = o_w.view(np.uint64), n_w.view(np.uint64)
    same = n_len == o_len
    o_same, n_same = np.repeat(same, o_len), np.repeat(same, n_len)
    if not ((o_dst[o_same] == n_dst[n_same]).all() and (o_et[o_same] == n_et[n_same]).all()
            and (o_wb[o_same] == n_wb[n_same]).all()):
        return None
    gone = []
    for i in np.flatnonzero(~same):                      # the shorter lists, link by link
        k, a1 = int(o_rp[i]), int(o_rp[i + 1])
        for j in range(int(n_rp[i]), int(n_rp[i + 1])):
            while k < a1 and not (o_dst[k] == n_dst[j] and o_et[k] == n_et[j] and o_wb[k] == n_wb[j]):
                gone.append(k)
                k += 1
            if k == a1:
                return None
            k += 1
        gone.extend(range(k, a1))
    return np.array(gone, dtype=np.int64)


def _removed_flat(flat, pos):
    """``flat`` (as ``Graph._flatten`` returns it) without the links at the flattened positions ``pos`` (distinct, any
    order), as rwr_graph_remove_links leaves the lists: new arrays, the other links in their order."""
    node_id, node_type, rowptr, o_dst, o_et, o_w = flat
    keep = np.ones(int(rowptr[-1]), dtype=bool)
    keep[pos] = False
    new_rowptr = rowptr - np.searchsorted(np.sort(pos), rowptr, side="left")
    return (node_id, node_type, new_rowptr.astype(np.int64), o_dst[keep], o_et[keep], o_w[keep])


def _removed_nodes_flat(flat, lost):
    """``flat`` (as ``Graph._flatten`` returns it) without the nodes ``lost`` (distinct indices, any order), as
    rwr_graph_remove_nodes leaves the graph: every link from or to a lost node gone, the other nodes closed up in their order
    and every remaining target renumbered.  Returns ``(new_flat, new_node_index, new_link_index)``, the two index arrays
    over the old nodes and the old flattened positions with -1 for what left."""
    node_id, node_type, rowptr, o_dst, o_et, o_w = flat
    n = int(node_id.shape[0])
    stay = np.ones(n, dtype=bool)
    stay[lost] = False
    new_node = np.where(stay, np.cumsum(stay) - 1, -1).astype(np.int32)
    src = np.repeat(np.arange(n), np.diff(rowptr))
    keep = stay[src] & stay[o_dst]
    new_link = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int64)
    new_rowptr = np.zeros(int(stay.sum()) + 1, dtype=np.int64)
    new_rowptr[1:] = np.cumsum(np.bincount(src[keep], minlength=n)[stay])
    new_flat = (node_id[stay], node_type[stay], new_rowptr, new_node[o_dst[keep]].astype(np.int32), o_et[keep], o_w[keep])
    return new_flat, new_node, new_link


def _lost_nodes(old_flat, new_flat):
    """The indices (in ``old_flat``, ascending) of the nodes by which ``old_flat`` exceeds ``new_flat``: the remaining nodes
    are unchanged and in order -- matched by (id, type), the earliest old node for each new one -- and, with the nodes mapped
    to their new indices, every remaining list is its old self minus the links to lost nodes, bitwise.  ``None`` otherwise
    (also when no node is missing).  Where nodes of equal (id, type) leave a choice that the earliest match gets wrong, the
    lists do not compare equal and the graph is sent whole."""
    o_id, o_type = old_flat[0], old_flat[1]
    n_id, n_type = new_flat[0], new_flat[1]
    n_old, n_new = int(o_id.shape[0]), int(n_id.shape[0])
    if n_new >= n_old or n_new == 0:
        return None
    lost, k = [], 0
    for j in range(n_new):
        while k < n_old and not (o_id[k] == n_id[j] and o_type[k] == n_type[j]):
            lost.append(k)
            k += 1
        if k == n_old:
            return None
        k += 1
    lost.extend(range(k, n_old))
    lost = np.array(lost, dtype=np.int32)
    want = _removed_nodes_flat(old_flat, lost)[0]
    for a, b in zip(want[2:], new_flat[2:]):
        if a.shape != b.shape:
            return None
    if not ((want[2] == new_flat[2]).all() and (want[3] == new_flat[3]).all() and (want[4] == new_flat[4]).all()
            and (want[5].view(np.uint64) == new_flat[5].view(np.uint64)).all()):
        return None
    return lost


class Graph:
    """class Graph (Graph.cs:37-94).  ``nodes``/``edges`` are the caller's dictionaries
    (kept by reference, Graph.cs:46-47); ``buildGraph()`` hands the RAW links to
    rwr_graph_create, which filters/normalises/transposes on the device."""

    incremental_rebuilds = 0     # buildGraph() calls (all instances) that went through rwr_graph_update_links
    append_rebuilds = 0          # ... and those that went through rwr_graph_append_links (lists that only grew)
    node_append_rebuilds = 0     # ... and through rwr_graph_append_nodes (nodes added at the end, lists that only grew)
    remove_rebuilds = 0          # ... and through rwr_graph_remove_links (lists that only shrank)
    node_remove_rebuilds = 0     # ... and through rwr_graph_remove_nodes (nodes lost, the others unchanged and in order)

    def __init__(self, nodes: Dict[int, Node], edges: Dict[int, List[ForwardLink]], *, mode: Optional[str] = None,
                 device: int = -1, tile_seeds: int = 0, tile_group: int = 0, profile: bool = False,
                 workspace_bytes: int = 0, seed_row_kernel: Optional[str] = None):
        self.nodes = nodes
        self.edges = edges
        self._graph_cache = None
        self._h = C.c_void_p()
        self._opts = _lib.rwr_opts(C.sizeof(_lib.rwr_opts), device,
                                   {None: -1, "exact": _lib.RWR_MODE_EXACT}[mode],
                                   tile_seeds, tile_group, 1 if profile else 0, workspace_bytes,
                                   {None: 0, "auto": 0, "fold": 1, "scan": 2, "simple": 3}[seed_row_kernel], 0)
        self._flat = None
        self._desc = None       # (rwr_graph_desc bytes of _flat: _marshal_graphs)
        self._sent = None
        self._sent_in_order = False   # the node dictionary enumerated its keys as 0, 1, ..., n-1 when _sent was taken

    # -- flat constructors (the layout of include/rwr.h), used by the bench for big graphs
    @classmethod
    def from_flat(cls, node_id, node_type, rowptr, dst, etype, w, **opts) -> "Graph":
        g = cls(None, None, **opts)
        g._flat = (np.ascontiguousarray(node_id, dtype=np.int64), np.ascontiguousarray(node_type, dtype=np.uint8),
                   np.ascontiguousarray(rowptr, dtype=np.int64), np.ascontiguousarray(dst, dtype=np.int32),
                   np.ascontiguousarray(etype, dtype=np.uint8), np.ascontiguousarray(w, dtype=np.float64))
        return g

    def _flatten(self):
        n = len(self.nodes)
        node_id = np.empty(n, dtype=np.int64)
        node_type = np.empty(n, dtype=np.uint8)
        for i in range(n):
            nd = self.nodes[i]                 # keys must be 0..n-1 (Graph.cs:52,55)
            node_id[i] = nd.id
            node_type[i] = int(nd.type)
        rowptr = np.zeros(n + 1, dtype=np.int64)
        for i in range(n):
            rowptr[i + 1] = rowptr[i] + (len(self.edges[i]) if i in self.edges else 0)
        m = int(rowptr[n])
        dst = np.empty(m, dtype=np.int32)
        etype = np.empty(m, dtype=np.uint8)
        w = np.empty(m, dtype=np.float64)
        e = 0
        for i in range(n):
            if i in self.edges:
                for l in self.edges[i]:
                    dst[e] = l.targetNode
                    etype[e] = int(l.type)
                    w[e] = l.weight
                    e += 1
        return node_id, node_type, rowptr, dst, etype, w

    def buildGraph(self) -> None:
        """Graph.buildGraph (Graph.cs:51-88) -> rwr_graph_create.

        Called again on the same object after the caller mutated its dictionaries (the harness relabels link types
        between runs, Experiment.cs:84-101): when nodes, list lengths and targets are unchanged, only the links whose
        type or weight differ are sent (rwr_graph_update_links); when the lists only grew at their ends, only the new links
        (rwr_graph_append_links); when, besides, the node dictionary gained keys at its end -- the old nodes unchanged and in
        the same order, the new keys continuing the index sequence -- only the new nodes and links (rwr_graph_append_nodes);
        when lists only lost links (``del edges[u][k]``: every shorter list a subsequence of its old self, the others
        unchanged) only the positions of the links that left (rwr_graph_remove_links);
        when the node dictionary only lost nodes -- the remaining ones unchanged, in order and re-keyed 0 .. n-1, every
        remaining list its old self minus the links to lost nodes, with the targets re-keyed alike -- only the lost indices
        (rwr_graph_remove_nodes);
        lists that grew AND whose old links changed, lists that shrank AND grew or changed, a changed old node or a reordered
        dictionary are sent whole.  The device state is the same either way."""
        lib = _lib.load()
        flat = self._flat if self._flat is not None else self._flatten()
        node_id, node_type, rowptr, dst, etype, w = flat
        if self._h and self._flat is None and self._sent is not None:
            o_id, o_type, o_rowptr, o_dst, o_etype, o_w = self._sent
            if (o_rowptr.shape == rowptr.shape and (o_rowptr == rowptr).all() and (o_dst == dst).all()
                    and (o_id == node_id).all() and (o_type == node_type).all()):
                changed = np.flatnonzero((o_etype != etype) | (o_w.view(np.uint64) != w.view(np.uint64))).astype(np.int64)
                self.updateLinks(changed, etype[changed], w[changed])
                self._sent = flat
                Graph.incremental_rebuilds += 1
                return
            grown = _grown_lists(self._sent, flat)
            if grown is not None:
                # (the library directly: appendLinks would merge the links into a copy of _sent, and flat IS that merge)
                s, t, et, ww = (np.ascontiguousarray(a) for a in grown)
                _lib.check(lib.rwr_graph_append_links(self._handle(), int(s.shape[0]), _p(s, C.c_int32), _p(t, C.c_int32),
                                                      _p(et, C.c_uint8), _p(ww, C.c_double), None))
                self._rowptr = rowptr
                self._sent = flat
                self._graph_cache = None
                Graph.append_rebuilds += 1
                return
            gone = _shrunk_lists(self._sent, flat)
            if gone is not None:
                # (the library directly, as above: flat IS _sent without those links)
                _lib.check(lib.rwr_graph_remove_links(self._handle(), int(gone.shape[0]), _p(gone, C.c_int64)))
                self._rowptr = rowptr
                self._sent = flat
                self._graph_cache = None
                Graph.remove_rebuilds += 1
                return
            more = _grown_nodes(self._sent, flat) if self._sent_in_order and self._keys_in_order() else None
            if more is not None:
                n_old, (s, t, et, ww) = more
                s, t, et, ww = (np.ascontiguousarray(a) for a in (s, t, et, ww))
                ids, types = np.ascontiguousarray(node_id[n_old:]), np.ascontiguousarray(node_type[n_old:])
                _lib.check(lib.rwr_graph_append_nodes(self._handle(), int(ids.shape[0]), _p(ids, C.c_int64), _p(types, C.c_uint8),
                                                      int(s.shape[0]), _p(s, C.c_int32), _p(t, C.c_int32), _p(et, C.c_uint8),
                                                      _p(ww, C.c_double), None))
                self._n = int(node_id.shape[0])
                self._rowptr = rowptr
                self._sent = flat
                self._graph_cache = None
                Graph.node_append_rebuilds += 1
                return
            lost = _lost_nodes(self._sent, flat)
            if lost is not None:
                # (the library directly: flat IS _sent without those nodes)
                _lib.check(lib.rwr_graph_remove_nodes(self._handle(), int(lost.shape[0]), _p(lost, C.c_int32), None, None, None))
                self._n = int(node_id.shape[0])
                self._rowptr = rowptr
                self._sent = flat
                self._graph_cache = None
                Graph.node_remove_rebuilds += 1
                return
        if self._h:
            lib.rwr_graph_destroy(self._h)
            self._h = C.c_void_p()
        self._n = int(node_id.shape[0])
        self._rowptr = rowptr
        _lib.check(lib.rwr_graph_create(self._n, _p(node_id, C.c_int64), _p(node_type, C.c_uint8),
                                        _p(rowptr, C.c_int64), _p(dst, C.c_int32), _p(etype, C.c_uint8),
                                        _p(w, C.c_double), C.byref(self._opts), C.byref(self._h)))
        self._sent = flat if self._flat is None else None     # (dictionary graphs: fresh arrays, kept for the next diff)
        self._sent_in_order = self._flat is None and self._keys_in_order()
        self._graph_cache = None

    def _keys_in_order(self) -> bool:
        """The node dictionary enumerates its keys as 0, 1, ..., n-1 (what a loader that only ever adds nodes leaves)."""
        return all(k == i for i, k in enumerate(self.nodes))

    def updateLinks(self, link_index, etype=None, w=None) -> None:
        """rwr_graph_update_links: new type / raw weight for the raw links at the given flattened positions, then the
        device-side rebuild.  (Flat graphs: the caller's arrays are not touched; keep them in step yourself.)"""
        idx = np.ascontiguousarray(link_index, dtype=np.int64)
        et = None if etype is None else np.ascontiguousarray(etype, dtype=np.uint8)
        ww = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
        if (et is not None and et.shape != idx.shape) or (ww is not None and ww.shape != idx.shape):
            raise ValueError("etype / w must have one entry per link index")
        _lib.check(_lib.load().rwr_graph_update_links(
            self._handle(), int(idx.shape[0]), _p(idx, C.c_int64),
            None if et is None else _p(et, C.c_uint8), None if ww is None else _p(ww, C.c_double)))
        self._graph_cache = None

    def appendLinks(self, src, dst, etype, w) -> np.ndarray:
        """rwr_graph_append_links: link q goes to the end of node src[q]'s list (edges[src].Add(...), Graph.cs:40), then the
        device-side rebuild.  Returns the positions of the new links in the new flattened raw list (for updateLinks); the
        link at old position e of row i is now at e + (appended links with src < i).

        The object's record of what the device holds follows.  A dictionary graph: the caller adds the same links to
        ``edges`` (this call does not touch the dictionaries) and the next buildGraph() finds nothing more to send.  A flat
        graph: the object continues with merged COPIES of the arrays; the caller's arrays are not touched."""
        s = np.ascontiguousarray(src, dtype=np.int32)
        t = np.ascontiguousarray(dst, dtype=np.int32)
        et = np.ascontiguousarray(etype, dtype=np.uint8)
        ww = np.ascontiguousarray(w, dtype=np.float64)
        if s.ndim != 1 or t.shape != s.shape or et.shape != s.shape or ww.shape != s.shape:
            raise ValueError("src / dst / etype / w must be one-dimensional and of one length")
        pos = np.zeros(s.shape[0], dtype=np.int64)
        _lib.check(_lib.load().rwr_graph_append_links(
            self._handle(), int(s.shape[0]), _p(s, C.c_int32), _p(t, C.c_int32), _p(et, C.c_uint8), _p(ww, C.c_double),
            _p(pos, C.c_int64)))
        if self._flat is not None:
            self._flat = _merged_flat(self._flat, s, t, et, ww, pos)
            self._desc = None
            self._rowptr = self._flat[2]
        else:
            if self._sent is not None:
                self._sent = _merged_flat(self._sent, s, t, et, ww, pos)
            rowptr = self._rowptr.copy()
            rowptr[1:] += np.cumsum(np.bincount(s, minlength=self._n).astype(np.int64))
            self._rowptr = rowptr
        self._graph_cache = None
        return pos

    def removeLinks(self, link_index) -> None:
        """rwr_graph_remove_links: the raw links at the given flattened positions (distinct, any order) leave their lists
        (edges[src].RemoveAt(k)), then the device-side rebuild.  Positions move: the surviving link at old position e is
        now at e - (removed positions < e).

        The object's record of what the device holds follows, as for appendLinks.  A dictionary graph: the caller deletes
        the same links from ``edges`` and the next buildGraph() finds nothing more to send.  A flat graph: the object
        continues with shortened COPIES of the arrays; the caller's arrays are not touched."""
        idx = np.ascontiguousarray(link_index, dtype=np.int64)
        if idx.ndim != 1:
            raise ValueError("link_index must be one-dimensional")
        _lib.check(_lib.load().rwr_graph_remove_links(self._handle(), int(idx.shape[0]), _p(idx, C.c_int64)))
        if self._flat is not None:
            self._flat = _removed_flat(self._flat, idx)
            self._desc = None
            self._rowptr = self._flat[2]
        else:
            if self._sent is not None:
                self._sent = _removed_flat(self._sent, idx)
            self._rowptr = self._rowptr - np.searchsorted(np.sort(idx), self._rowptr, side="left")
        self._graph_cache = None

    def removeNodes(self, node_index) -> Tuple[np.ndarray, np.ndarray]:
        """rwr_graph_remove_nodes: the nodes at the given indices (distinct, any order) leave the graph with every raw link
        from or to them (nodes.Remove(i); edges.Remove(i), and the links to i out of the other lists), the others close up
        and keep their order, then the device-side rebuild.  Returns ``(new_node_index, new_link_index)``: the new index
        of every old node and the new flattened position of every old link, -1 for what left.

        The object's record of what the device holds follows, as for removeLinks.  A dictionary graph: the caller takes
        the same nodes and links out of ``nodes`` / ``edges`` and re-keys both by ``new_node_index``; the next buildGraph()
        finds nothing more to send.  A flat graph: the object continues with shortened COPIES of the arrays."""
        idx = np.ascontiguousarray(node_index, dtype=np.int32)
        if idx.ndim != 1:
            raise ValueError("node_index must be one-dimensional")
        new_node = np.zeros(self._n, dtype=np.int32)
        new_link = np.zeros(int(self._rowptr[-1]), dtype=np.int64)
        _lib.check(_lib.load().rwr_graph_remove_nodes(self._handle(), int(idx.shape[0]), _p(idx, C.c_int32),
                                                      _p(new_node, C.c_int32), _p(new_link, C.c_int64), None))
        stay = new_node >= 0
        if self._flat is not None:
            self._flat = _removed_nodes_flat(self._flat, idx)[0]
            self._desc = None
            self._rowptr = self._flat[2]
        else:
            if self._sent is not None:
                self._sent = _removed_nodes_flat(self._sent, idx)[0]
            kept = np.concatenate([[0], np.cumsum(new_link >= 0)]).astype(np.int64)   # kept links in front of a position
            self._rowptr = np.concatenate([kept[self._rowptr[:-1][stay]], kept[-1:]])
        self._n = int(stay.sum())
        self._graph_cache = None
        return new_node, new_link

    def appendNodes(self, nodes, src=(), dst=(), etype=(), w=()) -> Tuple[int, np.ndarray]:
        """rwr_graph_append_nodes: node j of ``nodes`` (``Node`` objects or ``(id, type)`` pairs) gets index n + j and an empty
        list (nodes.Add(n + j, ...); edges.Add(n + j, new List<ForwardLink>()), Graph.cs:39-40); then the links are appended
        as appendLinks appends them, src and dst ranging over the grown node set; one device-side rebuild for both.  Returns
        ``(first_index, positions)``: the index of the first new node and the positions of the new links in the new
        flattened raw list.

        The object's record of what the device holds follows, as for appendLinks: the caller of a dictionary graph adds the
        same nodes and links to ``nodes`` / ``edges``; a flat graph continues with grown COPIES of its arrays."""
        pairs = [(nd.id, int(nd.type)) if isinstance(nd, Node) else (int(nd[0]), int(nd[1])) for nd in nodes]
        ids = np.ascontiguousarray([p[0] for p in pairs], dtype=np.int64)
        types = np.ascontiguousarray([p[1] for p in pairs], dtype=np.uint8)
        s = np.ascontiguousarray(src, dtype=np.int32)
        t = np.ascontiguousarray(dst, dtype=np.int32)
        et = np.ascontiguousarray(etype, dtype=np.uint8)
        ww = np.ascontiguousarray(w, dtype=np.float64)
        if s.ndim != 1 or t.shape != s.shape or et.shape != s.shape or ww.shape != s.shape:
            raise ValueError("src / dst / etype / w must be one-dimensional and of one length")
        first = self._n
        pos = np.zeros(s.shape[0], dtype=np.int64)
        _lib.check(_lib.load().rwr_graph_append_nodes(
            self._handle(), int(ids.shape[0]), _p(ids, C.c_int64), _p(types, C.c_uint8), int(s.shape[0]), _p(s, C.c_int32),
            _p(t, C.c_int32), _p(et, C.c_uint8), _p(ww, C.c_double), _p(pos, C.c_int64)))
        self._n = first + int(ids.shape[0])
        if self._flat is not None:
            self._flat = _merged_flat(_extended_flat(self._flat, ids, types), s, t, et, ww, pos)
            self._desc = None
            self._rowptr = self._flat[2]
        else:
            if self._sent is not None:
                self._sent = _merged_flat(_extended_flat(self._sent, ids, types), s, t, et, ww, pos)
            rowptr = np.concatenate([self._rowptr, np.full(int(ids.shape[0]), self._rowptr[-1], dtype=np.int64)])
            rowptr[1:] += np.cumsum(np.bincount(s, minlength=self._n).astype(np.int64))
            self._rowptr = rowptr
        self._graph_cache = None
        return first, pos

    def size(self) -> int:
        """Graph.size() (Graph.cs:91-93)."""
        return len(self.nodes) if self.nodes is not None else int(self._flat[0].shape[0])

    def _handle(self):
        if not self._h:
            raise RuntimeError("Graph.buildGraph() has not been called")
        return self._h

    def normalized(self) -> Tuple[np.ndarray, np.ndarray]:
        """(w_norm per raw link, dangling per node) -- rwr_graph_get_normalized."""
        lib = _lib.load()
        m = int(self._rowptr[-1])
        wn = np.zeros(max(m, 1), dtype=np.float64)
        dg = np.zeros(self._n, dtype=np.uint8)
        _lib.check(lib.rwr_graph_get_normalized(self._handle(), _p(wn, C.c_double), _p(dg, C.c_uint8)))
        return wn[:m], dg

    @property
    def graph(self) -> Dict[int, Optional[List[ForwardLink]]]:
        """The public field Graph.graph (Graph.cs:43): normalised explicit links per node,
        None for dangling nodes; materialised lazily from the device."""
        if self._graph_cache is None:
            wn, dg = self.normalized()
            out = {}
            flat = self._flat if self._flat is not None else self._flatten()
            _, _, rowptr, dst, etype, _ = flat
            for i in range(self._n):
                if dg[i]:
                    out[i] = None
                else:
                    out[i] = [ForwardLink(int(dst[e]), EdgeType(int(etype[e])), float(wn[e]))
                              for e in range(int(rowptr[i]), int(rowptr[i + 1])) if etype[e] != 0]
            self._graph_cache = out
        return self._graph_cache

    def stats(self) -> dict:
        st = _lib.rwr_stats()
        st.struct_size = C.sizeof(_lib.rwr_stats)
        _lib.check(_lib.load().rwr_get_stats(self._handle(), C.byref(st)))
        return {k: getattr(st, k) for k, _ in st._fields_}

    def reset_stats(self) -> None:
        _lib.check(_lib.load().rwr_reset_stats(self._handle()))

    def close(self) -> None:
        if self._h:
            _lib.load().rwr_graph_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):   # the reference types have no Dispose: release on finalisation
        try:
            self.close()
        except Exception:
            pass


def _desc_raw(flat) -> bytes:
    node_id, node_type, rowptr, dst, etype, w = flat
    return bytes(_lib.rwr_graph_desc(int(node_id.shape[0]), 0, _p(node_id, C.c_int64), _p(node_type, C.c_uint8),
                                     _p(rowptr, C.c_int64), _p(dst, C.c_int32), _p(etype, C.c_uint8), _p(w, C.c_double)))


def _marshal_graphs(graphs, testSets):
    """The arguments of rwr_eval_graphs for a batch: the descriptor array, the test sets as (ptr, ids), and the arrays that
    must stay alive during the call.  A Graph made from flat arrays keeps its descriptor (its six pointers) with the arrays,
    so that a batch of such graphs costs the interpreter one bytes.join -- with ten host threads behind one interpreter lock
    (bench.py --config C1) the per-graph ctypes conversions were most of the call."""
    K = len(graphs)
    alive, raw = [], []
    for g in graphs:
        if g._flat is not None:
            if g._desc is None:
                g._desc = _desc_raw(g._flat)
            raw.append(g._desc)
        else:
            flat = g._flatten()                 # (dictionary graphs: fresh arrays every time, the caller may have changed the lists)
            alive.append(flat)
            raw.append(_desc_raw(flat))
    descs = (_lib.rwr_graph_desc * max(K, 1))()
    if K:
        C.memmove(descs, b"".join(raw), K * C.sizeof(_lib.rwr_graph_desc))
    ptr = np.zeros(K + 1, dtype=np.int64)
    if K:
        np.cumsum(np.fromiter(map(len, testSets), dtype=np.int64, count=K), out=ptr[1:])
    total = int(ptr[K])
    if total == 0:
        ids = np.zeros(1, dtype=np.int64)
    elif all(isinstance(t, np.ndarray) for t in testSets):
        ids = np.ascontiguousarray(np.concatenate(testSets), dtype=np.int64)
    else:
        ids = np.fromiter(itertools.chain.from_iterable(testSets), dtype=np.int64, count=total)
    return descs, ptr, ids, alive


def EvaluateGraphs(graphs, seeds, dampingFactor: float, nIteration: int, testSets, *, device: int = -1):
    """The loop body of the reference's harness (Experiment.cs:69-134) for MANY graphs at once (rwr_eval_graphs):
    graphs[k].buildGraph(); Recommender(graphs[k]).RecommendationEval(seeds[k], d, T, testSets[k]) for every k, with one
    build launch, one iteration launch and one evaluation launch for all ego-network-sized graphs of the batch.  The Graph
    objects are NOT built by this call (no device handle is left behind).  Returns (nHits[K], sumPrecision[K], listLen[K])."""
    K = len(graphs)
    if len(seeds) != K or len(testSets) != K:
        raise ValueError("one seed and one test set per graph")
    descs, ptr, ids, _alive = _marshal_graphs(graphs, testSets)
    seeds_a = np.ascontiguousarray(seeds, dtype=np.int32)
    hits = np.zeros(K, dtype=np.int64)
    sp = np.zeros(K, dtype=np.float64)
    ln = np.zeros(K, dtype=np.int64)
    opts = _lib.rwr_opts(C.sizeof(_lib.rwr_opts), device, -1, 0, 0, 0, 0, 0, 0)
    _lib.check(_lib.load().rwr_eval_graphs(K, descs, _p(seeds_a, C.c_int32), C.c_float(dampingFactor), int(nIteration),
                                           _p(ptr, C.c_int64), _p(ids, C.c_int64), C.byref(opts), _p(hits, C.c_int64),
                                           _p(sp, C.c_double), _p(ln, C.c_int64)))
    return hits, sp, ln


class Model:
    """class Model (Model.cs:5-116) backed by rwr_model_run (rwr_model_run_restart once the host has edited restart)."""

    def __init__(self, graph: Graph, dampingFactor: float, targetNode: Optional[int] = None):
        self.graph = graph
        self.nNodes = graph.size()
        self.dampingFactor = float(dampingFactor)
        self._seed = -1 if targetNode is None else int(targetNode)
        n = self.nNodes
        if targetNode is None:                                  # Model.cs:14-31
            self.rank = np.ones(n)
            self.restart = np.full(n, 1.0 / n)
        else:                                                   # Model.cs:33-50
            self.rank = np.zeros(n)
            self.restart = np.zeros(n)
            if 0 <= targetNode < n:
                self.rank[targetNode] = float(n)
                self.restart[targetNode] = 1.0
        self.nextRank = np.zeros(n)
        self.iterations = 0

    def _ctor_state(self) -> bool:
        """rank / nextRank / restart are still what the constructor left (then the whole run can stay on the device)."""
        n = self.nNodes
        if self.nextRank.shape != (n,) or self.rank.shape != (n,) or np.any(self.nextRank != 0):
            return False
        if self._seed < 0:
            return bool(np.all(self.rank == 1.0))
        if not (0 <= self._seed < n):
            return bool(np.all(self.rank == 0.0))
        r = self.rank
        return bool(r[self._seed] == float(n) and np.count_nonzero(r) == (1 if n else 0))

    def _custom_restart(self) -> Optional[np.ndarray]:
        """The public field restart (Model.cs:12) as a contiguous float64 array when the host has edited it, else None
        (the constructor's one-hot / uniform vector, which the seed / global paths serve)."""
        n = self.nNodes
        v = np.ascontiguousarray(self.restart, dtype=np.float64)
        if v.shape != (n,):
            raise ValueError(f"Model.restart must hold {n} values")
        expect = np.full(n, 1.0 / n) if self._seed < 0 else np.zeros(n)
        if 0 <= self._seed < n:
            expect[self._seed] = 1.0
        return None if np.array_equal(v, expect) else v

    def run(self, arg=None) -> None:
        """run(int) / run(double) / run()  (Model.cs:68-73, 57-66, 52-55).  From the constructor's state the whole loop
        runs on the device (rwr_model_run); on a model that has already been advanced -- the reference's run() continues
        from the current rank -- it is driven step by step through deliverRanks / updateRanks / checkConvergence."""
        lib = _lib.load()
        if isinstance(arg, (int, np.integer)) and not isinstance(arg, bool):
            mode, value = _lib.RWR_RUN_ITERATIONS, float(arg)
        elif arg is None:
            mode, value = _lib.RWR_RUN_DEFAULT_THRESHOLD, 0.0
        else:
            mode, value = _lib.RWR_RUN_THRESHOLD, float(arg)
        v = self._custom_restart()
        if v is not None:
            # an edited restart vector: the whole loop on the device from the current rank (rwr_model_run_restart)
            if np.any(self.nextRank != 0):
                raise RuntimeError("run() on a non-zero nextRank (the reference would add on top of it): call updateRanks() first")
            rank = np.ascontiguousarray(self.rank, dtype=np.float64)
            out = np.empty(self.nNodes, dtype=np.float64)
            it = C.c_int64(0)
            _lib.check(lib.rwr_model_run_restart(self.graph._handle(), _p(v, C.c_double), _p(rank, C.c_double),
                                                 self.dampingFactor, mode, value, _p(out, C.c_double), C.byref(it)))
            self.rank = out
            self.nextRank = np.zeros(self.nNodes)
            self.iterations = int(it.value)
            return
        if not self._ctor_state():
            if mode == _lib.RWR_RUN_ITERATIONS:                  # Model.cs:68-73
                for _ in range(int(value)):
                    self.deliverRanks()
                    self.updateRanks()
                self.iterations = int(value)
                return
            threshold = (1.0 / 1.7976931348623157e308) * self.nNodes if mode == _lib.RWR_RUN_DEFAULT_THRESHOLD else value
            it = 0
            while True:                                          # Model.cs:57-66
                self.deliverRanks()
                it += 1
                done = self.checkConvergence(threshold)
                self.updateRanks()
                if done:
                    break
            self.iterations = it
            return
        out = np.zeros(self.nNodes, dtype=np.float64)
        it = C.c_int64(0)
        _lib.check(lib.rwr_model_run(self.graph._handle(), self._seed, self.dampingFactor, mode, value,
                                     _p(out, C.c_double), C.byref(it)))
        self.rank = out
        self.nextRank = np.zeros(self.nNodes)
        self.iterations = int(it.value)

    @staticmethod
    def RunBatch(graph: Graph, dampingFactor: float, seeds, arg=None) -> Tuple[np.ndarray, np.ndarray]:
        """K personalised models in one call (rwr_model_run_batch), an addition beside the reference surface:
        returns (ranks, iterations), ranks[k] / iterations[k] being what Model(graph, dampingFactor, seeds[k]).run(arg)
        leaves in rank / iterations.  arg as in run(): an int gives iterations, a float a threshold, None the default
        threshold (each seed then stops at its own convergence step)."""
        lib = _lib.load()
        if isinstance(arg, (int, np.integer)) and not isinstance(arg, bool):
            mode, value = _lib.RWR_RUN_ITERATIONS, float(arg)
        elif arg is None:
            mode, value = _lib.RWR_RUN_DEFAULT_THRESHOLD, 0.0
        else:
            mode, value = _lib.RWR_RUN_THRESHOLD, float(arg)
        s = np.ascontiguousarray(seeds, dtype=np.int32).reshape(-1)
        K, n = int(s.shape[0]), graph.size()
        ranks = np.zeros((K, n), dtype=np.float64)
        iters = np.zeros(K, dtype=np.int64)
        _lib.check(lib.rwr_model_run_batch(graph._handle(), _p(s, C.c_int32), K, float(dampingFactor), mode, value,
                                           _p(ranks, C.c_double), _p(iters, C.c_int64)))
        return ranks, iters

    @staticmethod
    def RunRestartBatch(graph: Graph, dampingFactor: float, restarts, starts=None, arg=None,
                        out: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray]:
        """K models with caller-set restart vectors in one call (rwr_model_run_restart_batch), an addition beside the
        reference surface: returns (ranks, iterations), ranks[k] / iterations[k] being what a Model whose restart field
        holds vector k leaves after run(arg).  restarts: a sequence of {node: weight} dicts or (indices, values) pairs;
        starts[k] >= 0: Model(graph, dampingFactor, starts[k]), -1 (or starts=None): Model(graph, dampingFactor).  arg as
        in RunBatch.  out: an optional (K, n) float64 array to receive the ranks."""
        lib = _lib.load()
        if isinstance(arg, (int, np.integer)) and not isinstance(arg, bool):
            mode, value = _lib.RWR_RUN_ITERATIONS, float(arg)
        elif arg is None:
            mode, value = _lib.RWR_RUN_DEFAULT_THRESHOLD, 0.0
        else:
            mode, value = _lib.RWR_RUN_THRESHOLD, float(arg)
        K, sup_ptr, sup_idx, sup_val, st = _pack_restarts(restarts, starts)
        n = graph.size()
        if out is None:
            ranks = np.zeros((K, n), dtype=np.float64)
        else:
            ranks = out
            if ranks.shape != (K, n) or ranks.dtype != np.float64 or not ranks.flags.c_contiguous:
                raise ValueError(f"out must be a C-contiguous float64 array of shape ({K}, {n})")
        iters = np.zeros(K, dtype=np.int64)
        _lib.check(lib.rwr_model_run_restart_batch(graph._handle(), K, _p(sup_ptr, C.c_int64), _p(sup_idx, C.c_int32),
                                                   _p(sup_val, C.c_double), None if st is None else _p(st, C.c_int32),
                                                   float(dampingFactor), mode, value, _p(ranks, C.c_double),
                                                   _p(iters, C.c_int64)))
        return ranks, iters

    def deliverRanks(self) -> None:
        """Model.deliverRanks (Model.cs:76-100): nextRank <- one propagation of the current rank (rwr_model_deliver)."""
        n = self.nNodes
        if np.any(self.nextRank != 0):
            raise RuntimeError("deliverRanks() on a non-zero nextRank (the reference would add on top of it): call updateRanks() first")
        v = self._custom_restart()
        rank = np.ascontiguousarray(self.rank, dtype=np.float64)
        out = np.empty(n, dtype=np.float64)
        if v is not None:
            _lib.check(_lib.load().rwr_model_deliver_restart(self.graph._handle(), _p(v, C.c_double), self.dampingFactor,
                                                             _p(rank, C.c_double), _p(out, C.c_double)))
        else:
            _lib.check(_lib.load().rwr_model_deliver(self.graph._handle(), self._seed, self.dampingFactor,
                                                     _p(rank, C.c_double), _p(out, C.c_double)))
        self.nextRank = out

    def updateRanks(self) -> None:
        """Model.updateRanks (Model.cs:103-108)."""
        self.rank = np.array(self.nextRank, dtype=np.float64)
        self.nextRank = np.zeros(self.nNodes)

    def checkConvergence(self, threshold: float) -> bool:
        """Model.checkConvergence (Model.cs:110-115): sequential sum of |rank - nextRank| < threshold."""
        if self.nNodes == 0:
            return 0.0 < threshold
        diff = np.cumsum(np.abs(np.asarray(self.rank, dtype=np.float64) - self.nextRank))   # cumsum adds left to right
        return bool(diff[-1] < threshold)


def _pack_restarts(restarts, starts):
    """K restart vectors -- {node: weight} dicts or (indices, values) pairs -- as the CSR arrays of the batched restart
    entries, and the start nodes as int32 (None stays None): (K, sup_ptr, sup_idx, sup_val, starts)."""
    idx, val, ptr = [], [], [0]
    for r in restarts:
        if isinstance(r, dict):
            i, v = list(r.keys()), list(r.values())
        else:
            i, v = r
        i = np.asarray(i, dtype=np.int32).reshape(-1)
        v = np.asarray(v, dtype=np.float64).reshape(-1)
        if i.shape != v.shape:
            raise ValueError("a restart vector's indices and values differ in length")
        idx.append(i)
        val.append(v)
        ptr.append(ptr[-1] + int(i.shape[0]))
    K = len(idx)
    sup_ptr = np.asarray(ptr, dtype=np.int64)
    sup_idx = np.ascontiguousarray(np.concatenate(idx) if K else np.zeros(0, dtype=np.int32), dtype=np.int32)
    sup_val = np.ascontiguousarray(np.concatenate(val) if K else np.zeros(0), dtype=np.float64)
    st = None
    if starts is not None:
        st = np.ascontiguousarray(starts, dtype=np.int32).reshape(-1)
        if st.shape[0] != K:
            raise ValueError(f"starts must hold {K} values")
    return K, sup_ptr, sup_idx, sup_val, st


class Recommender:
    """class Recommender (Recommender.cs:7-52)."""

    def __init__(self, graph: Graph):
        self.graph = graph

    def Recommendation(self, idxTargetUser: int, dampingFactor: float, nIteration: int,
                       topN: Optional[int] = None) -> List[Tuple[int, float]]:
        """Recommendation(int, float, int[, int topN]) -> list of (item id, score), i.e. the
        reference's List<KeyValuePair<long,double>> (Recommender.cs:14-40, 42-51)."""
        g = self.graph
        if g.edges is not None and idxTargetUser not in g.edges:
            raise KeyError(idxTargetUser)        # graph.edges[idxTargetUser], Recommender.cs:21
        lib = _lib.load()
        cap = g.size() if topN is None or topN <= 0 else min(g.size(), int(topN))
        ids = np.empty(max(cap, 1), dtype=np.int64)
        sc = np.empty(max(cap, 1), dtype=np.float64)
        cnt = C.c_int64(cap)
        _lib.check(lib.rwr_recommend(g._handle(), int(idxTargetUser), C.c_float(dampingFactor), int(nIteration),
                                     0 if topN is None else int(topN), _p(ids, C.c_int64), _p(sc, C.c_double),
                                     C.byref(cnt)))
        c = int(cnt.value)
        return list(zip(ids[:c].tolist(), sc[:c].tolist()))

    def RecommendationArrays(self, idxTargetUser: int, dampingFactor: float, nIteration: int,
                             topN: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
        """The same ranked list as Recommendation(), as two arrays (ids, scores) -- for graphs whose full list has
        millions of entries, where building Python tuples costs far more than the GPU call."""
        g = self.graph
        if g.edges is not None and idxTargetUser not in g.edges:
            raise KeyError(idxTargetUser)
        cap = g.size() if topN is None or topN <= 0 else min(g.size(), int(topN))
        ids = np.empty(max(cap, 1), dtype=np.int64)
        sc = np.empty(max(cap, 1), dtype=np.float64)
        cnt = C.c_int64(cap)
        _lib.check(_lib.load().rwr_recommend(g._handle(), int(idxTargetUser), C.c_float(dampingFactor), int(nIteration),
                                             0 if topN is None else int(topN), _p(ids, C.c_int64), _p(sc, C.c_double),
                                             C.byref(cnt)))
        c = int(cnt.value)
        return ids[:c], sc[:c]

    def RecommendationEval(self, idxTargetUser: int, dampingFactor: float, nIteration: int, testSet):
        """Recommendation + the harness's evaluation of it (Experiment.cs:109,121-128) without bringing the list
        to the host: returns (nHits, sumPrecision, len(list)); MAP contribution = sumPrecision / nHits."""
        g = self.graph
        if g.edges is not None and idxTargetUser not in g.edges:
            raise KeyError(idxTargetUser)
        t = np.ascontiguousarray(sorted(testSet), dtype=np.int64)
        hits, sp, ln = C.c_int64(0), C.c_double(0.0), C.c_int64(0)
        _lib.check(_lib.load().rwr_recommend_eval(g._handle(), int(idxTargetUser), C.c_float(dampingFactor),
                                                  int(nIteration), _p(t, C.c_int64), len(t), C.byref(hits),
                                                  C.byref(sp), C.byref(ln)))
        return int(hits.value), float(sp.value), int(ln.value)

    def RecommendationEvalBatch(self, seeds, dampingFactor: float, nIteration: int, testSets):
        """RecommendationEval for K seeds of this graph, each with its own test set (rwr_recommend_eval_batch):
        returns (nHits[K], sumPrecision[K], listLen[K])."""
        seeds = np.ascontiguousarray(seeds, dtype=np.int32)
        K = int(seeds.shape[0])
        if len(testSets) != K:
            raise ValueError("one test set per seed")
        ptr = np.zeros(K + 1, dtype=np.int64)
        for k, t in enumerate(testSets):
            ptr[k + 1] = ptr[k] + len(t)
        ids = np.ascontiguousarray([x for t in testSets for x in t], dtype=np.int64) if ptr[K] else np.zeros(1, dtype=np.int64)
        hits = np.zeros(K, dtype=np.int64)
        sp = np.zeros(K, dtype=np.float64)
        ln = np.zeros(K, dtype=np.int64)
        _lib.check(_lib.load().rwr_recommend_eval_batch(self.graph._handle(), _p(seeds, C.c_int32), K, C.c_float(dampingFactor),
                                                        int(nIteration), _p(ptr, C.c_int64), _p(ids, C.c_int64),
                                                        _p(hits, C.c_int64), _p(sp, C.c_double), _p(ln, C.c_int64)))
        return hits, sp, ln

    def RecommendationBatch(self, seeds, dampingFactor: float, nIteration: int, topN: int):
        """Batch entry (an addition, see include/rwr.h): (ids[K,topN], scores[K,topN], counts[K])."""
        lib = _lib.load()
        seeds = np.ascontiguousarray(seeds, dtype=np.int32)
        K = int(seeds.shape[0])
        ids = np.zeros((K, topN), dtype=np.int64)
        sc = np.zeros((K, topN), dtype=np.float64)
        counts = np.zeros(K, dtype=np.int32)
        _lib.check(lib.rwr_recommend_batch(self.graph._handle(), _p(seeds, C.c_int32), K, C.c_float(dampingFactor),
                                           int(nIteration), int(topN), _p(ids, C.c_int64), _p(sc, C.c_double),
                                           _p(counts, C.c_int32)))
        return ids, sc, counts

    def RecommendationTypedBatch(self, seeds, dampingFactor: float, nIteration: int, topN: int, candType,
                                 exclEdgeTypes=(), excludeSelf: bool = False):
        """Top-N lists among the nodes of one node type for K seeds (rwr_recommend_typed_batch, an addition, see
        include/rwr.h): (ids[K,topN], scores[K,topN], counts[K]).  candType: the candidates' NodeType; exclEdgeTypes: an
        iterable of EdgeType -- the targets of the seed's raw links of those types are no candidates; excludeSelf: neither is
        the seed.  "Who to follow" is (NodeType.USER, (EdgeType.FRIENDSHIP, EdgeType.FOLLOW), True)."""
        lib = _lib.load()
        seeds = np.ascontiguousarray(seeds, dtype=np.int32).reshape(-1)
        K = int(seeds.shape[0])
        mask = 0
        for t in exclEdgeTypes:
            mask |= 1 << int(EdgeType(t))
        topN = int(topN)
        ids = np.zeros((K, max(topN, 0)), dtype=np.int64)
        sc = np.zeros((K, max(topN, 0)), dtype=np.float64)
        counts = np.zeros(K, dtype=np.int32)
        _lib.check(lib.rwr_recommend_typed_batch(self.graph._handle(), _p(seeds, C.c_int32), K, C.c_float(dampingFactor),
                                                 int(nIteration), topN, int(candType), mask, 1 if excludeSelf else 0,
                                                 _p(ids, C.c_int64), _p(sc, C.c_double), _p(counts, C.c_int32)))
        return ids, sc, counts

    def RecommendationTyped(self, idxTargetNode: int, dampingFactor: float, nIteration: int, topN: int, candType,
                            exclEdgeTypes=(), excludeSelf: bool = False) -> List[Tuple[int, float]]:
        """RecommendationTypedBatch for one seed, as Recommendation returns its list: [(node id, score), ...]."""
        ids, sc, counts = self.RecommendationTypedBatch([int(idxTargetNode)], dampingFactor, nIteration, topN, candType,
                                                        exclEdgeTypes, excludeSelf)
        c = int(counts[0])
        return list(zip(ids[0, :c].tolist(), sc[0, :c].tolist()))

    def RecommendationTypedEvalBatch(self, seeds, dampingFactor: float, nIteration: int, testSets, candType, exclEdgeTypes=(),
                                     excludeSelf: bool = False, topN: int = 0):
        """Hits and the running-precision sum (Experiment.cs:121-128) of K seeds' WHOLE lists among the nodes of one node type
        against one test set each, evaluated on the device without writing a ranked list (rwr_recommend_typed_eval_batch, an
        addition, see include/rwr.h): (nHits[K], sumPrecision[K], listLen[K]).  candType, exclEdgeTypes and excludeSelf as in
        RecommendationTypedBatch; testSets: a sequence of K collections of node ids; topN > 0 evaluates the first topN entries
        of every list (any value: there is no 1024 limit here), topN <= 0 the whole list."""
        lib = _lib.load()
        seeds = np.ascontiguousarray(seeds, dtype=np.int32).reshape(-1)
        K = int(seeds.shape[0])
        mask = 0
        for t in exclEdgeTypes:
            mask |= 1 << int(EdgeType(t))
        tests = [np.asarray(list(t), dtype=np.int64).reshape(-1) for t in testSets]
        if len(tests) != K:
            raise ValueError(f"testSets must hold {K} id collections")
        tp = np.zeros(K + 1, dtype=np.int64)
        tp[1:] = np.cumsum([len(t) for t in tests])
        ti = np.ascontiguousarray(np.concatenate(tests) if K else np.zeros(0, dtype=np.int64), dtype=np.int64)
        hits = np.zeros(K, dtype=np.int64)
        sp = np.zeros(K, dtype=np.float64)
        ln = np.zeros(K, dtype=np.int64)
        _lib.check(lib.rwr_recommend_typed_eval_batch(self.graph._handle(), _p(seeds, C.c_int32), K, C.c_float(dampingFactor),
                                                      int(nIteration), int(topN), int(candType), mask, 1 if excludeSelf else 0,
                                                      _p(tp, C.c_int64), _p(ti, C.c_int64), _p(hits, C.c_int64),
                                                      _p(sp, C.c_double), _p(ln, C.c_int64)))
        return hits, sp, ln

    def RecommendationTypedEval(self, idxTargetNode: int, dampingFactor: float, nIteration: int, testSet, candType,
                                exclEdgeTypes=(), excludeSelf: bool = False, topN: int = 0) -> Tuple[int, float, int]:
        """RecommendationTypedEvalBatch for one seed, as RecommendationEval returns: (nHits, sumPrecision, len(list))."""
        hits, sp, ln = self.RecommendationTypedEvalBatch([int(idxTargetNode)], dampingFactor, nIteration, [testSet], candType,
                                                         exclEdgeTypes, excludeSelf, topN)
        return int(hits[0]), float(sp[0]), int(ln[0])

    def RecommendationTypedPositionsBatch(self, seeds, dampingFactor: float, nIteration: int, testSets, candType,
                                          exclEdgeTypes=(), excludeSelf: bool = False):
        """The 0-based position and the score of every test id in K seeds' WHOLE lists among the nodes of one node type, found
        on the device by counting, no list written (rwr_recommend_typed_positions_batch, an addition, see include/rwr.h):
        (positions, scores, listLen[K]).  positions and scores are lists of K arrays aligned with testSets -- entry by entry,
        in the caller's order, duplicates kept; -1 / +0.0 where the list does not hold the id.  candType, exclEdgeTypes and
        excludeSelf as in RecommendationTypedBatch.  Any ranking metric follows on the host, for instance
        MRR = mean(1 / (p[p >= 0].min() + 1)) and NDCG@10 = sum(1 / log2(p[(p >= 0) & (p < 10)] + 2)) / ideal."""
        lib = _lib.load()
        seeds = np.ascontiguousarray(seeds, dtype=np.int32).reshape(-1)
        K = int(seeds.shape[0])
        mask = 0
        for t in exclEdgeTypes:
            mask |= 1 << int(EdgeType(t))
        tp, ti, pos, sc, ln = _pack_tests(testSets, K)
        _lib.check(lib.rwr_recommend_typed_positions_batch(self.graph._handle(), _p(seeds, C.c_int32), K, C.c_float(dampingFactor),
                                                           int(nIteration), int(candType), mask, 1 if excludeSelf else 0,
                                                           _p(tp, C.c_int64), _p(ti, C.c_int64), _p(pos, C.c_int64),
                                                           _p(sc, C.c_double), _p(ln, C.c_int64)))
        return _split_tests(tp, pos), _split_tests(tp, sc), ln

    def RecommendationTypedPositions(self, idxTargetNode: int, dampingFactor: float, nIteration: int, testSet, candType,
                                     exclEdgeTypes=(), excludeSelf: bool = False):
        """RecommendationTypedPositionsBatch for one seed: (positions, scores, len(list)), the arrays aligned with testSet."""
        pos, sc, ln = self.RecommendationTypedPositionsBatch([int(idxTargetNode)], dampingFactor, nIteration, [testSet], candType,
                                                             exclEdgeTypes, excludeSelf)
        return pos[0], sc[0], int(ln[0])

    def RecommendationFilteredBatch(self, seeds, dampingFactor: float, nIteration: int, topN: int, candType=None,
                                    exclEdgeTypes=(), excludeSelf: bool = False, pool=None, deny=None):
        """Top-N lists for K seeds within a candidate pool the caller sets and with a deny list per seed
        (rwr_recommend_filtered_batch, an addition, see include/rwr.h): (ids[K,topN], scores[K,topN], counts[K]).  candType: the
        candidates' NodeType, None: nodes of any type; exclEdgeTypes and excludeSelf as in RecommendationTypedBatch; pool: an
        iterable of node INDICES, any order, duplicates allowed -- only these are ranked, for every seed (None: no pool, []: an
        empty pool, every list empty); deny: K iterables of node indices, list k never shown to seed k (None: none)."""
        lib = _lib.load()
        seeds = np.ascontiguousarray(seeds, dtype=np.int32).reshape(-1)
        K = int(seeds.shape[0])
        mask = 0
        for t in exclEdgeTypes:
            mask |= 1 << int(EdgeType(t))
        pc, pi, dp, di = _pack_filter(pool, deny, K)
        topN = int(topN)
        ids = np.zeros((K, max(topN, 0)), dtype=np.int64)
        sc = np.zeros((K, max(topN, 0)), dtype=np.float64)
        counts = np.zeros(K, dtype=np.int32)
        _lib.check(lib.rwr_recommend_filtered_batch(self.graph._handle(), _p(seeds, C.c_int32), K, C.c_float(dampingFactor),
                                                    int(nIteration), topN, -1 if candType is None else int(candType), mask,
                                                    1 if excludeSelf else 0, pc, None if pi is None else _p(pi, C.c_int32),
                                                    None if dp is None else _p(dp, C.c_int64),
                                                    None if di is None else _p(di, C.c_int32), _p(ids, C.c_int64),
                                                    _p(sc, C.c_double), _p(counts, C.c_int32)))
        return ids, sc, counts

    def RecommendationFiltered(self, idxTargetNode: int, dampingFactor: float, nIteration: int, topN: int, candType=None,
                               exclEdgeTypes=(), excludeSelf: bool = False, pool=None, deny=None) -> List[Tuple[int, float]]:
        """RecommendationFilteredBatch for one seed, as Recommendation returns its list: [(node id, score), ...]; deny: the
        seed's one deny list (an iterable of node indices) or None."""
        ids, sc, counts = self.RecommendationFilteredBatch([int(idxTargetNode)], dampingFactor, nIteration, topN, candType,
                                                           exclEdgeTypes, excludeSelf, pool, None if deny is None else [deny])
        c = int(counts[0])
        return list(zip(ids[0, :c].tolist(), sc[0, :c].tolist()))

    def RecommendationFilteredPositionsBatch(self, seeds, dampingFactor: float, nIteration: int, testSets, candType=None,
                                             exclEdgeTypes=(), excludeSelf: bool = False, pool=None, deny=None):
        """The 0-based position and the score of every test id in K seeds' WHOLE filtered lists
        (rwr_recommend_filtered_positions_batch, an addition, see include/rwr.h): (positions, scores, listLen[K]) as
        RecommendationTypedPositionsBatch returns them, over the lists RecommendationFilteredBatch defines.  A denied id, an id
        outside the pool and an id no node carries answer -1 / +0.0."""
        lib = _lib.load()
        seeds = np.ascontiguousarray(seeds, dtype=np.int32).reshape(-1)
        K = int(seeds.shape[0])
        mask = 0
        for t in exclEdgeTypes:
            mask |= 1 << int(EdgeType(t))
        pc, pi, dp, di = _pack_filter(pool, deny, K)
        tp, ti, pos, sc, ln = _pack_tests(testSets, K)
        _lib.check(lib.rwr_recommend_filtered_positions_batch(
            self.graph._handle(), _p(seeds, C.c_int32), K, C.c_float(dampingFactor), int(nIteration),
            -1 if candType is None else int(candType), mask, 1 if excludeSelf else 0, pc, None if pi is None else _p(pi, C.c_int32),
            None if dp is None else _p(dp, C.c_int64), None if di is None else _p(di, C.c_int32), _p(tp, C.c_int64),
            _p(ti, C.c_int64), _p(pos, C.c_int64), _p(sc, C.c_double), _p(ln, C.c_int64)))
        return _split_tests(tp, pos), _split_tests(tp, sc), ln

    def RecommendationCappedBatch(self, seeds, dampingFactor: float, nIteration: int, topN: int, candType=None, exclEdgeTypes=(),
                                  excludeSelf: bool = False, pool=None, deny=None, groupOf=None, groupCap: int = 1):
        """RecommendationFilteredBatch with a diversity cap: at most groupCap entries per group of nodes in every list
        (rwr_recommend_capped_batch, an addition, see include/rwr.h): (ids[K,topN], scores[K,topN], counts[K]).  groupOf: one
        int label per node of the graph (appended nodes included), any value >= 0 a group, a negative value "never capped";
        None: no cap, the filtered call.  groupCap in [1, 8].  Candidates the mask, excludeSelf, the pool or a deny list remove
        do not use up a group's allowance."""
        lib = _lib.load()
        seeds = np.ascontiguousarray(seeds, dtype=np.int32).reshape(-1)
        K = int(seeds.shape[0])
        mask = 0
        for t in exclEdgeTypes:
            mask |= 1 << int(EdgeType(t))
        pc, pi, dp, di = _pack_filter(pool, deny, K)
        go = _pack_groups(groupOf)
        if go is not None and go.shape[0] < self.graph.stats()["n"]:
            raise ValueError("groupOf must hold one label per node of the graph")
        topN = int(topN)
        ids = np.zeros((K, max(topN, 0)), dtype=np.int64)
        sc = np.zeros((K, max(topN, 0)), dtype=np.float64)
        counts = np.zeros(K, dtype=np.int32)
        _lib.check(lib.rwr_recommend_capped_batch(self.graph._handle(), _p(seeds, C.c_int32), K, C.c_float(dampingFactor),
                                                  int(nIteration), topN, -1 if candType is None else int(candType), mask,
                                                  1 if excludeSelf else 0, pc, None if pi is None else _p(pi, C.c_int32),
                                                  None if dp is None else _p(dp, C.c_int64),
                                                  None if di is None else _p(di, C.c_int32),
                                                  None if go is None else _p(go, C.c_int32), int(groupCap), _p(ids, C.c_int64),
                                                  _p(sc, C.c_double), _p(counts, C.c_int32)))
        return ids, sc, counts

    def RecommendationCapped(self, idxTargetNode: int, dampingFactor: float, nIteration: int, topN: int, candType=None,
                             exclEdgeTypes=(), excludeSelf: bool = False, pool=None, deny=None, groupOf=None,
                             groupCap: int = 1) -> List[Tuple[int, float]]:
        """RecommendationCappedBatch for one seed, as Recommendation returns its list: [(node id, score), ...]; deny: the
        seed's one deny list (an iterable of node indices) or None."""
        ids, sc, counts = self.RecommendationCappedBatch([int(idxTargetNode)], dampingFactor, nIteration, topN, candType,
                                                         exclEdgeTypes, excludeSelf, pool, None if deny is None else [deny],
                                                         groupOf, groupCap)
        c = int(counts[0])
        return list(zip(ids[0, :c].tolist(), sc[0, :c].tolist()))

    def RecommendationExplainedBatch(self, seeds, dampingFactor: float, nIteration: int, topN: int, nWhy: int = 3, candType=None,
                                     exclEdgeTypes=(), excludeSelf: bool = False, pool=None, deny=None, groupOf=None,
                                     groupCap: int = 1, wantNodes: bool = True, wantTotal: bool = True):
        """RecommendationCappedBatch with the reasons of every list entry (rwr_recommend_explained_batch, an addition, see
        include/rwr.h): (ids[K,topN], scores[K,topN], counts[K], nodes[K,topN], whySrc[K,topN,nWhy], whyTerm[K,topN,nWhy],
        whyTotal[K,topN]).  nodes: the entries' node indices (-1 behind a list's end); whySrc / whyTerm: the source node and the
        value of each entry's nWhy largest in-link addends fl(fl((1 - d) * previousRank[u]) * weight(u -> v)), largest first,
        -1 / +0.0 where an entry has fewer positive addends; whyTotal: the number of positive addends.  nWhy in [0, 8].
        wantNodes / wantTotal False: that table is not computed and None is returned in its place; with nWhy 0 and both False
        the call is the capped call."""
        lib = _lib.load()
        seeds = np.ascontiguousarray(seeds, dtype=np.int32).reshape(-1)
        K = int(seeds.shape[0])
        mask = 0
        for t in exclEdgeTypes:
            mask |= 1 << int(EdgeType(t))
        pc, pi, dp, di = _pack_filter(pool, deny, K)
        go = _pack_groups(groupOf)
        if go is not None and go.shape[0] < self.graph.stats()["n"]:
            raise ValueError("groupOf must hold one label per node of the graph")
        topN, nWhy = int(topN), int(nWhy)
        width, r = max(topN, 0), min(max(nWhy, 0), 8)
        ids = np.zeros((K, width), dtype=np.int64)
        sc = np.zeros((K, width), dtype=np.float64)
        counts = np.zeros(K, dtype=np.int32)
        nodes = np.full((K, width), -1, dtype=np.int32) if wantNodes else None
        src = np.full((K, width, r), -1, dtype=np.int32)
        term = np.zeros((K, width, r), dtype=np.float64)
        total = np.zeros((K, width), dtype=np.int64) if wantTotal else None
        _lib.check(lib.rwr_recommend_explained_batch(
            self.graph._handle(), _p(seeds, C.c_int32), K, C.c_float(dampingFactor), int(nIteration), topN,
            -1 if candType is None else int(candType), mask, 1 if excludeSelf else 0, pc, None if pi is None else _p(pi, C.c_int32),
            None if dp is None else _p(dp, C.c_int64), None if di is None else _p(di, C.c_int32),
            None if go is None else _p(go, C.c_int32), int(groupCap), nWhy, _p(ids, C.c_int64), _p(sc, C.c_double),
            _p(counts, C.c_int32), None if nodes is None else _p(nodes, C.c_int32), _p(src, C.c_int32), _p(term, C.c_double),
            None if total is None else _p(total, C.c_int64)))
        return ids, sc, counts, nodes, src, term, total

    def RecommendationExplained(self, idxTargetNode: int, dampingFactor: float, nIteration: int, topN: int, nWhy: int = 3,
                                candType=None, exclEdgeTypes=(), excludeSelf: bool = False, pool=None, deny=None, groupOf=None,
                                groupCap: int = 1):
        """RecommendationExplainedBatch for one seed: ([(node id, score), ...], nodes[count], whySrc[count,nWhy],
        whyTerm[count,nWhy], whyTotal[count]); deny: the seed's one deny list (an iterable of node indices) or None."""
        ids, sc, counts, nodes, src, term, total = self.RecommendationExplainedBatch(
            [int(idxTargetNode)], dampingFactor, nIteration, topN, nWhy, candType, exclEdgeTypes, excludeSelf, pool,
            None if deny is None else [deny], groupOf, groupCap)
        c = int(counts[0])
        return list(zip(ids[0, :c].tolist(), sc[0, :c].tolist())), nodes[0, :c], src[0, :c], term[0, :c], total[0, :c]

    def AudienceBatch(self, targets, d: float, n_iter: int, cand_type=None, etype_mask=(), exclude_self: bool = False,
                      top_n: int = 100):
        """The audiences of K targets (rwr_recommend_audience_batch, an addition, see include/rwr.h): (ids[K,top_n],
        scores[K,top_n], nodes[K,top_n], counts[K]).  List k ranks the nodes s of NodeType cand_type (None: of any type) by the
        score a walk of n_iter steps FROM s gives targets[k]; the nodes with a raw link to targets[k] whose EdgeType is in
        etype_mask (an iterable of EdgeType, or the mask as an int) are left out, targets[k] too with exclude_self.  targets:
        node indices, taken as they are (any type, repeats allowed).  nodes: the entries' node indices, -1 behind a list's end.
        The scores agree with the forward walks' to the tolerance the header derives, not bitwise."""
        lib = _lib.load()
        targets = np.ascontiguousarray(targets, dtype=np.int32).reshape(-1)
        K = int(targets.shape[0])
        if isinstance(etype_mask, (int, np.integer)):
            mask = int(etype_mask)
        else:
            mask = 0
            for t in etype_mask:
                mask |= 1 << int(EdgeType(t))
        top_n = int(top_n)
        width = max(top_n, 0)
        ids = np.zeros((K, width), dtype=np.int64)
        sc = np.zeros((K, width), dtype=np.float64)
        nodes = np.full((K, width), -1, dtype=np.int32)
        counts = np.zeros(K, dtype=np.int32)
        _lib.check(lib.rwr_recommend_audience_batch(self.graph._handle(), K, _p(targets, C.c_int32), C.c_float(d), int(n_iter),
                                                    -1 if cand_type is None else int(cand_type), mask, 1 if exclude_self else 0,
                                                    top_n, _p(ids, C.c_int64), _p(sc, C.c_double), _p(nodes, C.c_int32),
                                                    _p(counts, C.c_int32)))
        return ids, sc, nodes, counts

    def Audience(self, target: int, d: float, n_iter: int, cand_type=None, etype_mask=(), exclude_self: bool = False,
                 top_n: int = 100) -> List[Tuple[int, float]]:
        """AudienceBatch for one target, as Recommendation returns its list: [(node id, score), ...]."""
        ids, sc, _, counts = self.AudienceBatch([int(target)], d, n_iter, cand_type, etype_mask, exclude_self, top_n)
        c = int(counts[0])
        return list(zip(ids[0, :c].tolist(), sc[0, :c].tolist()))

    @staticmethod
    def _pack_target_sets(sets, weights):
        """K target sets as the audience set entries take them: (K, set_ptr, set_idx, set_w or None).  sets: K iterables of
        node indices; weights: None (every weight 1.0) or K iterables parallel to the sets."""
        members = [np.ascontiguousarray(m if isinstance(m, np.ndarray) else list(m), dtype=np.int32).reshape(-1) for m in sets]
        K = len(members)
        sp = np.zeros(K + 1, dtype=np.int64)
        sp[1:] = np.cumsum([len(m) for m in members])
        si = np.ascontiguousarray(np.concatenate(members + [np.zeros(0, dtype=np.int32)]), dtype=np.int32)
        if si.shape[0] == 0:
            si = np.zeros(1, dtype=np.int32)
        sw = None
        if weights is not None:
            ws = [np.ascontiguousarray(w if isinstance(w, np.ndarray) else list(w), dtype=np.float64).reshape(-1) for w in weights]
            if len(ws) != K or any(len(w) != len(m) for w, m in zip(ws, members)):
                raise ValueError("weights must hold one weight per member of every set")
            sw = np.ascontiguousarray(np.concatenate(ws + [np.zeros(0)]), dtype=np.float64)
            if sw.shape[0] == 0:
                sw = np.zeros(1, dtype=np.float64)
        return K, sp, si, sw

    @staticmethod
    def _edge_mask(etype_mask):
        if isinstance(etype_mask, (int, np.integer)):
            return int(etype_mask)
        mask = 0
        for t in etype_mask:
            mask |= 1 << int(EdgeType(t))
        return mask

    def AudienceSetBatch(self, sets, d: float, n_iter: int, weights=None, cand_type=None, etype_mask=(),
                         exclude_members: bool = False, pool=None, deny=None, top_n: int = 100):
        """The audiences of K weighted target sets (rwr_recommend_audience_set_batch, an addition, see include/rwr.h):
        (ids[K,top_n], scores[K,top_n], nodes[K,top_n], counts[K]).  sets: K iterables of node indices (any type, any order;
        a member that repeats has its weights added); weights: None for 1.0 each, or K iterables parallel to the sets.  List k
        ranks the nodes s of cand_type (None: any type) by the weighted sum of the scores a walk of n_iter steps FROM s gives
        the members; the nodes with a raw link of a masked EdgeType to any member are left out, the members too with
        exclude_members, the node indices of deny[k], and with a pool (an iterable of node indices, [] for an empty one)
        every node outside it."""
        lib = _lib.load()
        K, sp, si, sw = self._pack_target_sets(sets, weights)
        pc, pi, dp, di = _pack_filter(pool, deny, K)
        top_n = int(top_n)
        width = max(top_n, 0)
        ids = np.zeros((K, width), dtype=np.int64)
        sc = np.zeros((K, width), dtype=np.float64)
        nodes = np.full((K, width), -1, dtype=np.int32)
        counts = np.zeros(K, dtype=np.int32)
        _lib.check(lib.rwr_recommend_audience_set_batch(
            self.graph._handle(), K, _p(sp, C.c_int64), _p(si, C.c_int32), None if sw is None else _p(sw, C.c_double), C.c_float(d),
            int(n_iter), -1 if cand_type is None else int(cand_type), self._edge_mask(etype_mask), 1 if exclude_members else 0, pc,
            None if pi is None else _p(pi, C.c_int32), None if dp is None else _p(dp, C.c_int64),
            None if di is None else _p(di, C.c_int32), top_n, _p(ids, C.c_int64), _p(sc, C.c_double), _p(nodes, C.c_int32),
            _p(counts, C.c_int32)))
        return ids, sc, nodes, counts

    def AudienceSet(self, members, d: float, n_iter: int, weights=None, cand_type=None, etype_mask=(),
                    exclude_members: bool = False, pool=None, deny=None, top_n: int = 100) -> List[Tuple[int, float]]:
        """AudienceSetBatch for one set, as Recommendation returns its list: [(node id, score), ...]; deny: the set's one deny
        list (an iterable of node indices) or None."""
        ids, sc, _, counts = self.AudienceSetBatch([members], d, n_iter, None if weights is None else [weights], cand_type,
                                                   etype_mask, exclude_members, pool, None if deny is None else [deny], top_n)
        c = int(counts[0])
        return list(zip(ids[0, :c].tolist(), sc[0, :c].tolist()))

    def AudienceSetPositionsBatch(self, sets, d: float, n_iter: int, testSets, weights=None, cand_type=None, etype_mask=(),
                                  exclude_members: bool = False, pool=None, deny=None):
        """The 0-based position and the score of every test id in K sets' WHOLE audience lists
        (rwr_recommend_audience_set_positions_batch, an addition, see include/rwr.h): (positions, scores, listLen[K]) as
        RecommendationFilteredPositionsBatch returns them, over the lists AudienceSetBatch defines.  An id the list does not
        hold answers -1 / +0.0."""
        lib = _lib.load()
        K, sp, si, sw = self._pack_target_sets(sets, weights)
        pc, pi, dp, di = _pack_filter(pool, deny, K)
        tp, ti, pos, sc, ln = _pack_tests(testSets, K)
        _lib.check(lib.rwr_recommend_audience_set_positions_batch(
            self.graph._handle(), K, _p(sp, C.c_int64), _p(si, C.c_int32), None if sw is None else _p(sw, C.c_double), C.c_float(d),
            int(n_iter), -1 if cand_type is None else int(cand_type), self._edge_mask(etype_mask), 1 if exclude_members else 0, pc,
            None if pi is None else _p(pi, C.c_int32), None if dp is None else _p(dp, C.c_int64),
            None if di is None else _p(di, C.c_int32), _p(tp, C.c_int64), _p(ti, C.c_int64), _p(pos, C.c_int64), _p(sc, C.c_double),
            _p(ln, C.c_int64)))
        return _split_tests(tp, pos), _split_tests(tp, sc), ln

    def RecommendationLongBatch(self, seeds, dampingFactor: float, nIteration: int, topN: int, candType=None, exclEdgeTypes=(),
                                excludeSelf: bool = False, pool=None, deny=None, groupOf=None, groupCap: int = 1,
                                wantNodes: bool = True):
        """RecommendationCappedBatch for lists of up to 65 536 entries (rwr_recommend_long_batch, an addition, see
        include/rwr.h): (ids[K,topN], scores[K,topN], counts[K], nodes[K,topN]).  The order is score descending, id descending,
        node index ascending; nodes: the entries' node indices (-1 behind a list's end), None with wantNodes False.  Up to
        1 024 entries the call is the explained call without reasons; candidate generation for a re-ranker is what the longer
        lists are for."""
        lib = _lib.load()
        seeds = np.ascontiguousarray(seeds, dtype=np.int32).reshape(-1)
        K = int(seeds.shape[0])
        mask = 0
        for t in exclEdgeTypes:
            mask |= 1 << int(EdgeType(t))
        pc, pi, dp, di = _pack_filter(pool, deny, K)
        go = _pack_groups(groupOf)
        if go is not None and go.shape[0] < self.graph.stats()["n"]:
            raise ValueError("groupOf must hold one label per node of the graph")
        topN = int(topN)
        width = max(topN, 0)
        ids = np.zeros((K, width), dtype=np.int64)
        sc = np.zeros((K, width), dtype=np.float64)
        counts = np.zeros(K, dtype=np.int32)
        nodes = np.full((K, width), -1, dtype=np.int32) if wantNodes else None
        _lib.check(lib.rwr_recommend_long_batch(
            self.graph._handle(), _p(seeds, C.c_int32), K, C.c_float(dampingFactor), int(nIteration), topN,
            -1 if candType is None else int(candType), mask, 1 if excludeSelf else 0, pc, None if pi is None else _p(pi, C.c_int32),
            None if dp is None else _p(dp, C.c_int64), None if di is None else _p(di, C.c_int32),
            None if go is None else _p(go, C.c_int32), int(groupCap), _p(ids, C.c_int64), _p(sc, C.c_double),
            _p(counts, C.c_int32), None if nodes is None else _p(nodes, C.c_int32)))
        return ids, sc, counts, nodes

    def RecommendationLong(self, idxTargetNode: int, dampingFactor: float, nIteration: int, topN: int, candType=None,
                           exclEdgeTypes=(), excludeSelf: bool = False, pool=None, deny=None, groupOf=None,
                           groupCap: int = 1) -> List[Tuple[int, float]]:
        """RecommendationLongBatch for one seed, as Recommendation returns its list: [(node id, score), ...]; deny: the seed's
        one deny list (an iterable of node indices) or None."""
        ids, sc, counts, _ = self.RecommendationLongBatch([int(idxTargetNode)], dampingFactor, nIteration, topN, candType,
                                                          exclEdgeTypes, excludeSelf, pool, None if deny is None else [deny],
                                                          groupOf, groupCap, False)
        c = int(counts[0])
        return list(zip(ids[0, :c].tolist(), sc[0, :c].tolist()))

    def AudienceSetLongBatch(self, sets, d: float, n_iter: int, weights=None, cand_type=None, etype_mask=(),
                             exclude_members: bool = False, pool=None, deny=None, top_n: int = 4096):
        """AudienceSetBatch for lists of up to 65 536 entries (rwr_recommend_audience_set_long_batch, an addition, see
        include/rwr.h): (ids[K,top_n], scores[K,top_n], nodes[K,top_n], counts[K]).  Up to 1 024 entries it returns
        AudienceSetBatch's arrays; a longer list continues that list."""
        lib = _lib.load()
        K, sp, si, sw = self._pack_target_sets(sets, weights)
        pc, pi, dp, di = _pack_filter(pool, deny, K)
        top_n = int(top_n)
        width = max(top_n, 0)
        ids = np.zeros((K, width), dtype=np.int64)
        sc = np.zeros((K, width), dtype=np.float64)
        nodes = np.full((K, width), -1, dtype=np.int32)
        counts = np.zeros(K, dtype=np.int32)
        _lib.check(lib.rwr_recommend_audience_set_long_batch(
            self.graph._handle(), K, _p(sp, C.c_int64), _p(si, C.c_int32), None if sw is None else _p(sw, C.c_double), C.c_float(d),
            int(n_iter), -1 if cand_type is None else int(cand_type), self._edge_mask(etype_mask), 1 if exclude_members else 0, pc,
            None if pi is None else _p(pi, C.c_int32), None if dp is None else _p(dp, C.c_int64),
            None if di is None else _p(di, C.c_int32), top_n, _p(ids, C.c_int64), _p(sc, C.c_double), _p(nodes, C.c_int32),
            _p(counts, C.c_int32)))
        return ids, sc, nodes, counts

    def AudienceSetLong(self, members, d: float, n_iter: int, weights=None, cand_type=None, etype_mask=(),
                        exclude_members: bool = False, pool=None, deny=None, top_n: int = 4096) -> List[Tuple[int, float]]:
        """AudienceSetLongBatch for one set, as Recommendation returns its list: [(node id, score), ...]; deny: the set's one
        deny list (an iterable of node indices) or None."""
        ids, sc, _, counts = self.AudienceSetLongBatch([members], d, n_iter, None if weights is None else [weights], cand_type,
                                                       etype_mask, exclude_members, pool, None if deny is None else [deny], top_n)
        c = int(counts[0])
        return list(zip(ids[0, :c].tolist(), sc[0, :c].tolist()))

    def RecommendationCappedPositionsBatch(self, seeds, dampingFactor: float, nIteration: int, testSets, candType=None,
                                           exclEdgeTypes=(), excludeSelf: bool = False, pool=None, deny=None, groupOf=None,
                                           groupCap: int = 1):
        """The 0-based position and the score of every test id in K seeds' WHOLE capped lists
        (rwr_recommend_capped_positions_batch, an addition, see include/rwr.h): (positions, scores, listLen[K]) as
        RecommendationFilteredPositionsBatch returns them, over the lists RecommendationCappedBatch defines.  An id the cap
        drops answers -1 / +0.0, like a denied one; listLen[k] is the capped list's length."""
        lib = _lib.load()
        seeds = np.ascontiguousarray(seeds, dtype=np.int32).reshape(-1)
        K = int(seeds.shape[0])
        mask = 0
        for t in exclEdgeTypes:
            mask |= 1 << int(EdgeType(t))
        pc, pi, dp, di = _pack_filter(pool, deny, K)
        go = _pack_groups(groupOf)
        if go is not None and go.shape[0] < self.graph.stats()["n"]:
            raise ValueError("groupOf must hold one label per node of the graph")
        tp, ti, pos, sc, ln = _pack_tests(testSets, K)
        _lib.check(lib.rwr_recommend_capped_positions_batch(
            self.graph._handle(), _p(seeds, C.c_int32), K, C.c_float(dampingFactor), int(nIteration),
            -1 if candType is None else int(candType), mask, 1 if excludeSelf else 0, pc, None if pi is None else _p(pi, C.c_int32),
            None if dp is None else _p(dp, C.c_int64), None if di is None else _p(di, C.c_int32),
            None if go is None else _p(go, C.c_int32), int(groupCap), _p(tp, C.c_int64), _p(ti, C.c_int64), _p(pos, C.c_int64),
            _p(sc, C.c_double), _p(ln, C.c_int64)))
        return _split_tests(tp, pos), _split_tests(tp, sc), ln

    def RecommendationRestartTypedPositionsBatch(self, restarts, starts, dampingFactor: float, nIteration: int, testSets, candType,
                                                 exclEdgeTypes=(), excludeMembers: bool = False, exclude=None):
        """RecommendationTypedPositionsBatch for K walks with caller-set restart vectors
        (rwr_recommend_restart_typed_positions_batch, an addition, see include/rwr.h): (positions, scores, listLen[K]) in the
        whole lists RecommendationRestartTypedBatch defines.  restarts, starts, candType, exclEdgeTypes, excludeMembers and
        exclude as there; testSets as in RecommendationTypedPositionsBatch."""
        lib = _lib.load()
        K, sup_ptr, sup_idx, sup_val, st = _pack_restarts(restarts, starts)
        ep = ei = None
        if exclude is not None:
            sets = [np.asarray(e, dtype=np.int32).reshape(-1) for e in exclude]
            if len(sets) != K:
                raise ValueError(f"exclude must hold {K} node lists")
            ep = np.zeros(K + 1, dtype=np.int64)
            ep[1:] = np.cumsum([len(e) for e in sets])
            ei = np.ascontiguousarray(np.concatenate(sets) if K else np.zeros(0, dtype=np.int32), dtype=np.int32)
        mask = 0
        for t in exclEdgeTypes:
            mask |= 1 << int(EdgeType(t))
        tp, ti, pos, sc, ln = _pack_tests(testSets, K)
        _lib.check(lib.rwr_recommend_restart_typed_positions_batch(
            self.graph._handle(), K, _p(sup_ptr, C.c_int64), _p(sup_idx, C.c_int32), _p(sup_val, C.c_double),
            None if st is None else _p(st, C.c_int32), None if ep is None else _p(ep, C.c_int64),
            None if ei is None else _p(ei, C.c_int32), float(dampingFactor), int(nIteration), int(candType), mask,
            1 if excludeMembers else 0, _p(tp, C.c_int64), _p(ti, C.c_int64), _p(pos, C.c_int64), _p(sc, C.c_double),
            _p(ln, C.c_int64)))
        return _split_tests(tp, pos), _split_tests(tp, sc), ln

    def RecommendationRestartTypedBatch(self, restarts, starts, dampingFactor: float, nIteration: int, topN: int, candType,
                                        exclEdgeTypes=(), excludeMembers: bool = False, exclude=None):
        """Top-N lists among the nodes of one node type for K walks with caller-set restart vectors
        (rwr_recommend_restart_typed_batch, an addition, see include/rwr.h): (ids[K,topN], scores[K,topN], counts[K]).
        restarts, starts and exclude as in RecommendationRestartBatch; candType and exclEdgeTypes as in
        RecommendationTypedBatch -- the targets of the raw links of those types of every member of set k are no candidates;
        excludeMembers: neither are the members themselves.  "Whom should this group follow" is (NodeType.USER,
        (EdgeType.FRIENDSHIP, EdgeType.FOLLOW), True)."""
        lib = _lib.load()
        K, sup_ptr, sup_idx, sup_val, st = _pack_restarts(restarts, starts)
        ep = ei = None
        if exclude is not None:
            sets = [np.asarray(e, dtype=np.int32).reshape(-1) for e in exclude]
            if len(sets) != K:
                raise ValueError(f"exclude must hold {K} node lists")
            ep = np.zeros(K + 1, dtype=np.int64)
            ep[1:] = np.cumsum([len(e) for e in sets])
            ei = np.ascontiguousarray(np.concatenate(sets) if K else np.zeros(0, dtype=np.int32), dtype=np.int32)
        mask = 0
        for t in exclEdgeTypes:
            mask |= 1 << int(EdgeType(t))
        topN = int(topN)
        ids = np.zeros((K, max(topN, 0)), dtype=np.int64)
        sc = np.zeros((K, max(topN, 0)), dtype=np.float64)
        counts = np.zeros(K, dtype=np.int32)
        _lib.check(lib.rwr_recommend_restart_typed_batch(self.graph._handle(), K, _p(sup_ptr, C.c_int64), _p(sup_idx, C.c_int32),
                                                         _p(sup_val, C.c_double), None if st is None else _p(st, C.c_int32),
                                                         None if ep is None else _p(ep, C.c_int64),
                                                         None if ei is None else _p(ei, C.c_int32), float(dampingFactor),
                                                         int(nIteration), topN, int(candType), mask, 1 if excludeMembers else 0,
                                                         _p(ids, C.c_int64), _p(sc, C.c_double), _p(counts, C.c_int32)))
        return ids, sc, counts

    def RecommendationRestartBatch(self, restarts, starts, dampingFactor: float, nIteration: int, topN: int, exclude=None):
        """Top-N lists of K walks with caller-set restart vectors, ranked on the device (rwr_recommend_restart_batch, an
        addition, see include/rwr.h): (ids[K,topN], scores[K,topN], counts[K]).  restarts and starts as in
        Model.RunRestartBatch (non-negative weights).  exclude: a sequence of K node lists -- the items their members LIKE
        are not candidates of vector k; None: the nodes of vector k's own support."""
        lib = _lib.load()
        K, sup_ptr, sup_idx, sup_val, st = _pack_restarts(restarts, starts)
        ep = ei = None
        if exclude is not None:
            sets = [np.asarray(e, dtype=np.int32).reshape(-1) for e in exclude]
            if len(sets) != K:
                raise ValueError(f"exclude must hold {K} node lists")
            ep = np.zeros(K + 1, dtype=np.int64)
            ep[1:] = np.cumsum([len(e) for e in sets])
            ei = np.ascontiguousarray(np.concatenate(sets) if K else np.zeros(0, dtype=np.int32), dtype=np.int32)
        topN = int(topN)
        ids = np.zeros((K, max(topN, 0)), dtype=np.int64)
        sc = np.zeros((K, max(topN, 0)), dtype=np.float64)
        counts = np.zeros(K, dtype=np.int32)
        _lib.check(lib.rwr_recommend_restart_batch(self.graph._handle(), K, _p(sup_ptr, C.c_int64), _p(sup_idx, C.c_int32),
                                                   _p(sup_val, C.c_double), None if st is None else _p(st, C.c_int32),
                                                   None if ep is None else _p(ep, C.c_int64),
                                                   None if ei is None else _p(ei, C.c_int32), float(dampingFactor),
                                                   int(nIteration), topN, _p(ids, C.c_int64), _p(sc, C.c_double),
                                                   _p(counts, C.c_int32)))
        return ids, sc, counts

    def RecommendationRestartEvalBatch(self, restarts, starts, dampingFactor: float, nIteration: int, testSets, topN: int = 0,
                                       exclude=None):
        """Hits and the running-precision sum (Experiment.cs:121-128) of K walks with caller-set restart vectors against one
        test set each, evaluated on the device without writing a ranked list (rwr_recommend_restart_eval_batch, an addition,
        see include/rwr.h): (nHits[K], sumPrecision[K], listLen[K]).  restarts, starts and exclude as in
        RecommendationRestartBatch; testSets: a sequence of K collections of item ids; topN > 0 evaluates the first topN
        entries of every list (Hits@N / AP@N), topN <= 0 the whole list."""
        lib = _lib.load()
        K, sup_ptr, sup_idx, sup_val, st = _pack_restarts(restarts, starts)
        ep = ei = None
        if exclude is not None:
            sets = [np.asarray(e, dtype=np.int32).reshape(-1) for e in exclude]
            if len(sets) != K:
                raise ValueError(f"exclude must hold {K} node lists")
            ep = np.zeros(K + 1, dtype=np.int64)
            ep[1:] = np.cumsum([len(e) for e in sets])
            ei = np.ascontiguousarray(np.concatenate(sets) if K else np.zeros(0, dtype=np.int32), dtype=np.int32)
        tests = [np.asarray(list(t), dtype=np.int64).reshape(-1) for t in testSets]
        if len(tests) != K:
            raise ValueError(f"testSets must hold {K} id collections")
        tp = np.zeros(K + 1, dtype=np.int64)
        tp[1:] = np.cumsum([len(t) for t in tests])
        ti = np.ascontiguousarray(np.concatenate(tests) if K else np.zeros(0, dtype=np.int64), dtype=np.int64)
        hits = np.zeros(K, dtype=np.int64)
        sp = np.zeros(K, dtype=np.float64)
        ln = np.zeros(K, dtype=np.int64)
        _lib.check(lib.rwr_recommend_restart_eval_batch(self.graph._handle(), K, _p(sup_ptr, C.c_int64), _p(sup_idx, C.c_int32),
                                                        _p(sup_val, C.c_double), None if st is None else _p(st, C.c_int32),
                                                        None if ep is None else _p(ep, C.c_int64),
                                                        None if ei is None else _p(ei, C.c_int32), float(dampingFactor),
                                                        int(nIteration), int(topN), _p(tp, C.c_int64), _p(ti, C.c_int64),
                                                        _p(hits, C.c_int64), _p(sp, C.c_double), _p(ln, C.c_int64)))
        return hits, sp, ln
