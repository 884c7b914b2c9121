"""Restart-vector walks ranked among the nodes of any type (rwr_recommend_restart_typed_batch /
Recommender.RecommendationRestartTypedBatch).  The expectation is the composition the header states, built from
verified pieces: the row rwr_model_run_restart returns for the vector (tests/test_gpu_restart_rank.py's _single_row), then the
candidates filtered and sorted here with sorted(key=(-score, -id)).  Ids must be equal, scores bitwise equal.

Graphs: tests/test_gpu_typed.py's mixed graph (users linked by FRIENDSHIP and FOLLOW, two dangling users), a graph whose hub
user's raw list spans two exclusion segments, and tests/test_gpu_restart_rank.py's 5 000-item graph for the identity."""
import ctypes as C

import numpy as np
import pytest

from tests import graphgen as gg
from tests.test_gpu_restart_rank import D, PD, PI32, PI64, _check, _packed, _single_row, _vectors, _sets, bits
from tests.test_gpu_typed import EXCLUDE_SEG_MAX, SEL_MAX_K, _flat, _lists, _mixed

pytestmark = pytest.mark.gpu

EXACT_MAX = 256
FOLLOWS = (gg.EDGE_FRIENDSHIP, gg.EDGE_FOLLOW)


@pytest.fixture(scope="module")
def amd():
    import recommendersystems_amd as m
    from recommendersystems_amd import _lib
    assert _lib.load().rwr_device_count() >= 1, "no gfx950 device: the HIP path cannot run"
    return m


def ranked_list(g, row, members, cand_type, edge_types, exclude_members):
    """the whole list the header defines for one vector: (ids, scores)"""
    out = set()
    for m in members:
        for p in range(int(g["rowptr"][m]), int(g["rowptr"][m + 1])):
            if int(g["etype"][p]) in edge_types:
                out.add(int(g["dst"][p]))
    if exclude_members:
        out |= {int(m) for m in members}
    cand = [(int(g["node_id"][i]), float(row[i])) for i in range(len(row)) if g["node_type"][i] == cand_type and i not in out]
    cand.sort(key=lambda c: (-c[1], -c[0]))
    return np.array([c[0] for c in cand], dtype=np.int64), np.array([c[1] for c in cand], dtype=np.float64)


class Case:
    """a graph, its vectors, explicit exclusion sets, and the single calls' rows per step count"""

    def __init__(self, amd, g, restarts, starts, sets, **opts):
        self.amd, self.g, self.restarts, self.starts, self.sets = amd, g, restarts, np.asarray(starts, dtype=np.int32), sets
        self.n = len(g["node_id"])
        self.G = amd.Graph.from_flat(**g, **opts)
        self.G.buildGraph()
        self._rows = {}

    def close(self):
        self.G.close()

    def row(self, k, T):
        if (k, T) not in self._rows:
            idx, val = self.restarts[k]
            self._rows[(k, T)] = _single_row(self.G, self.n, idx, val, int(self.starts[k]), D, T)
        return self._rows[(k, T)]

    def want(self, ks, T, top_n, cand_type, edge_types, members, explicit):
        return _packed([ranked_list(self.g, self.row(k, T), self.sets[k] if explicit else self.restarts[k][0], cand_type,
                                    set(edge_types), members) for k in ks], top_n)

    def call(self, ks, T, top_n, cand_type, edge_types, members, explicit, H=None):
        rec = self.amd.Recommender(H or self.G)
        return rec.RecommendationRestartTypedBatch([self.restarts[k] for k in ks], self.starts[list(ks)], D, T, top_n, cand_type,
                                                   edge_types, members, exclude=[self.sets[k] for k in ks] if explicit else None)


@pytest.fixture(scope="module")
def mixed_case(amd):
    g, (linkless, undef_only) = _mixed(11, uniform=False)
    rng = np.random.default_rng(8)
    restarts, starts = _vectors(g, 120, 19, rng)
    sets = _sets(restarts, 120, rng)
    # a dangling member in a support and in an explicit set; a start node that is a member, and one that is not
    restarts[4] = (np.array([linkless, 3, 9], dtype=np.int32), np.array([0.5, 1.0, 0.25]))
    sets[7] = np.array([undef_only, linkless, 5], dtype=np.int32)
    starts[4], starts[5] = 3, 11
    assert any(len(s) != len(np.unique(s)) for s in sets) and any(len(s) == 0 for s in sets) and any(len(i) == 0 for i, _ in restarts)
    c = Case(amd, g, restarts, starts, sets, tile_seeds=4, tile_group=1)
    c.linkless = linkless
    yield c
    c.close()


@pytest.mark.parametrize("K", [2, 19])
def test_whom_should_the_group_follow(mixed_case, K):
    c = mixed_case
    ks = list(range(K)) if K == 19 else [4, 7]
    for T in (0, 1, 10):
        for top_n in (1, 10, SEL_MAX_K):
            for members in (False, True):
                for explicit in (False, True):
                    got = c.call(ks, T, top_n, gg.NODE_USER, FOLLOWS, members, explicit)
                    want = c.want(ks, T, top_n, gg.NODE_USER, FOLLOWS, members, explicit)
                    _check(got, want, (K, T, top_n, members, explicit))
                    ids, sc, cnt = got                               # fewer candidates than top_n: a zero-filled tail
                    for k in range(K):
                        assert not ids[k, cnt[k]:].any() and not bits(sc[k, cnt[k]:]).any()
    # exclude_members drops the members of the type, the dangling one included, and nothing else
    for explicit in (False, True):
        off = c.want(ks, 10, SEL_MAX_K, gg.NODE_USER, (), False, explicit)
        on = c.want(ks, 10, SEL_MAX_K, gg.NODE_USER, (), True, explicit)
        for j, k in enumerate(ks):
            mem = np.unique(c.sets[k] if explicit else c.restarts[k][0])
            assert off[2][j] - on[2][j] == int((c.g["node_type"][mem] == gg.NODE_USER).sum())
    assert int(c.g["node_id"][c.linkless]) not in c.call([4], 10, SEL_MAX_K, gg.NODE_USER, (), True, False)[0][0].tolist()


def test_other_types_and_masks(mixed_case):
    c = mixed_case
    ks = list(range(19))
    for cand, mask, members in ((gg.NODE_ITEM, (), True), (gg.NODE_ITEM, (gg.EDGE_LIKE, gg.EDGE_UNDEFINED, gg.EDGE_AUTHORSHIP), False),
                                (gg.NODE_ETC, (gg.EDGE_MENTION,), True), (gg.NODE_UNDEFINED, tuple(range(8)), True), (77, FOLLOWS, True)):
        for explicit in (False, True):
            got = c.call(ks, 5, 30, cand, mask, members, explicit)
            _check(got, c.want(ks, 5, 30, cand, mask, members, explicit), (cand, mask, members, explicit))
    ids, sc, cnt = c.call(ks, 5, 30, 77, FOLLOWS, True, False)      # a type no node carries: the zeroed tables
    assert not cnt.any() and not ids.any() and not bits(sc).any()


def test_fallback_classes(amd, mixed_case):
    """K == 1 and a support of more than RWR_RESTART_EXACT_MAX entries run vector by vector and pass through the same end"""
    c = mixed_case
    for k in (0, 4, 7):
        for members in (False, True):
            got = c.call([k], 10, 25, gg.NODE_USER, FOLLOWS, members, k == 7)
            _check(got, c.want([k], 10, 25, gg.NODE_USER, FOLLOWS, members, k == 7), ("K == 1", k, members))
    rng = np.random.default_rng(9)
    wide_idx = rng.choice(c.n, EXACT_MAX + 1, replace=False).astype(np.int32)
    restarts = [c.restarts[1], (wide_idx, rng.random(EXACT_MAX + 1) + 0.1), c.restarts[4]]
    sets = [c.sets[1], np.array([0, 5, 5], dtype=np.int32), c.sets[4]]
    w = Case(amd, c.g, restarts, [-1, 7, 3], sets, tile_seeds=4, tile_group=1)
    for T in (1, 10):
        for members in (False, True):
            for explicit in (False, True):
                got = w.call([0, 1, 2], T, 40, gg.NODE_USER, FOLLOWS, members, explicit)
                _check(got, w.want([0, 1, 2], T, 40, gg.NODE_USER, FOLLOWS, members, explicit), ("wide", T, members, explicit))
    w.close()


def test_hub_member_two_segments(amd):
    g = gg.random_graph(31, n_users=300, n_items=80, n_likes=700, n_friend=100)
    lists = _lists(g)
    hub, lonely = 0, 299
    lists[hub] = [(1 + k % 297, gg.EDGE_FOLLOW if k % 3 else gg.EDGE_FRIENDSHIP, 1.0) for k in range(EXCLUDE_SEG_MAX)]
    lists[hub].append((lonely, gg.EDGE_FOLLOW, 1.0))
    lists[lonely].append((5, gg.EDGE_FRIENDSHIP, 1.0))
    g = _flat(g["node_id"], g["node_type"], lists)
    assert g["rowptr"][hub + 1] - g["rowptr"][hub] == EXCLUDE_SEG_MAX + 1
    restarts = [(np.array([hub, 298], dtype=np.int32), np.array([1.0, 2.0])), (np.array([17, 40], dtype=np.int32), np.array([1.0, 1.0])),
                (np.array([3], dtype=np.int32), np.array([1.0]))]
    sets = [np.array([298], dtype=np.int32), np.array([hub, hub], dtype=np.int32), np.zeros(0, dtype=np.int32)]
    c = Case(amd, g, restarts, [-1, hub, -1], sets, tile_seeds=4, tile_group=1)
    for explicit in (False, True):
        for members in (False, True):
            got = c.call([0, 1, 2], 2, 300, gg.NODE_USER, FOLLOWS, members, explicit)
            want = c.want([0, 1, 2], 2, 300, gg.NODE_USER, FOLLOWS, members, explicit)
            _check(got, want, ("hub", explicit, members))
    # the hub follows everybody but 298 (and itself): its group is left with those two, or with nobody
    assert c.want([0], 2, 300, gg.NODE_USER, FOLLOWS, False, False)[2][0] == 2
    assert c.want([0], 2, 300, gg.NODE_USER, FOLLOWS, True, False)[2][0] == 0
    c.close()


def test_item_like_is_recommend_restart_batch(amd, mixed_case):
    c = mixed_case
    rec = amd.Recommender(c.G)
    for K in (1, 2, 19):
        for T in (0, 10):
            for top_n in (1, 10, SEL_MAX_K):
                for explicit in (False, True):
                    ex = [c.sets[k] for k in range(K)] if explicit else None
                    want = rec.RecommendationRestartBatch(c.restarts[:K], c.starts[:K], D, T, top_n, exclude=ex)
                    got = rec.RecommendationRestartTypedBatch(c.restarts[:K], c.starts[:K], D, T, top_n, gg.NODE_ITEM,
                                                              (gg.EDGE_LIKE,), False, exclude=ex)
                    _check(got, want, ("identity", K, T, top_n, explicit))
    # more items than the select kernels' candidate slots
    g = gg.random_graph(31, n_users=300, n_items=5000, n_likes=9000, n_etc=6, n_friend=250, n_mention=120, n_author=60)
    rng = np.random.default_rng(5)
    restarts, starts = _vectors(g, 300, 19, rng)
    G = amd.Graph.from_flat(**g, tile_seeds=4, tile_group=1)
    G.buildGraph()
    rec = amd.Recommender(G)
    for top_n in (100, SEL_MAX_K):
        want = rec.RecommendationRestartBatch(restarts, starts, D, 10, top_n)
        _check(rec.RecommendationRestartTypedBatch(restarts, starts, D, 10, top_n, gg.NODE_ITEM, (gg.EDGE_LIKE,), False), want,
               ("identity, 5 000 items", top_n))
    G.close()


def test_refusals_write_nothing(amd, mixed_case):
    from recommendersystems_amd import _lib
    lib = _lib.load()
    name = b"rwr_recommend_restart_typed_batch"
    c = mixed_case
    n, h = c.n, c.G._handle()
    K, top_n = 3, 6
    ptr = np.array([0, 2, 3, 5], dtype=np.int64)
    idx = np.array([0, 5, 9, 3, 7], dtype=np.int32)
    val = np.array([1.0, 2.0, 1.0, 0.5, 0.5])
    start = np.array([-1, 9, 0], dtype=np.int32)
    eptr = np.array([0, 1, 1, 3], dtype=np.int64)
    eidx = np.array([5, 3, 3], dtype=np.int32)
    ids, sc, cnt = np.full((K, top_n), -77, dtype=np.int64), np.full((K, top_n), -7.5), np.full(K, -9, dtype=np.int32)
    pp, pi, pv, ps = ptr.ctypes.data_as(PI64), idx.ctypes.data_as(PI32), val.ctypes.data_as(PD), start.ctypes.data_as(PI32)
    pe, px = eptr.ctypes.data_as(PI64), eidx.ctypes.data_as(PI32)
    po, pc, pn = ids.ctypes.data_as(PI64), sc.ctypes.data_as(PD), cnt.ctypes.data_as(PI32)

    def call(handle=h, k=K, p=pp, i=pi, v=pv, s=ps, e=pe, x=px, d=D, T=3, top=top_n, cand=gg.NODE_USER, mask=0x0c, mem=1, o=po, q=pc,
             m=pn):
        return lib.rwr_recommend_restart_typed_batch(handle, k, p, i, v, s, e, x, d, T, top, cand, mask, mem, o, q, m), lib.rwr_last_error()

    def untouched():
        return (ids == -77).all() and (sc == -7.5).all() and (cnt == -9).all()

    st, msg = call(handle=None, k=-1, top=0, cand=999)
    assert st == _lib.RWR_E_INVALID and b"NULL graph" in msg
    assert call(k=0)[0] == _lib.RWR_OK and untouched()
    assert call(k=0, p=None, o=None, q=None, m=None, cand=999, top=0)[0] == _lib.RWR_OK
    for kw, word in ((dict(k=-1), b"negative K"), (dict(p=None), b"NULL"), (dict(o=None), b"NULL"), (dict(q=None), b"NULL"),
                     (dict(m=None), b"NULL"), (dict(top=0), b"top_n"), (dict(cand=-1), b"cand_type"), (dict(cand=256), b"cand_type"),
                     (dict(mask=1 << 8), b"excl_edge_mask"), (dict(mask=0x80000000), b"excl_edge_mask"), (dict(i=None), b"NULL"),
                     (dict(x=None), b"NULL excl_idx")):
        st, msg = call(**kw)
        assert st == _lib.RWR_E_INVALID and name in msg and word in msg, (kw, st, msg)
        assert untouched(), kw
    st, msg = call(top=SEL_MAX_K + 1)
    assert st == _lib.RWR_E_UNSUPPORTED and name in msg and b"1024" in msg and untouched()
    # what rwr_recommend_restart_batch reports for the vectors and the sets, with the same status and the batch position
    def edited(arr, at, value, status, words):
        keep = arr[at]
        arr[at] = value
        st, msg = call()
        arr[at] = keep
        assert st == status and name in msg and all(w in msg for w in words), (at, value, st, msg)
        assert untouched()

    edited(ptr, 0, 1, _lib.RWR_E_INVALID, (b"sup_ptr[0]",))
    edited(ptr, 2, 1, _lib.RWR_E_INVALID, (b"sup_ptr decreases", b"batch position 1"))
    edited(idx, 2, n, _lib.RWR_E_RANGE, (b"batch position 1",))
    edited(idx, 4, 3, _lib.RWR_E_INVALID, (b"twice", b"vector 2"))
    edited(start, 1, n, _lib.RWR_E_RANGE, (b"start", b"batch position 1"))
    edited(val, 3, float("inf"), _lib.RWR_E_UNSUPPORTED, (b"not finite", b"batch position 2"))
    edited(val, 0, -1.0, _lib.RWR_E_UNSUPPORTED, (b"negative", b"batch position 0"))
    edited(eptr, 0, 1, _lib.RWR_E_INVALID, (b"excl_ptr[0]",))
    edited(eptr, 2, 0, _lib.RWR_E_INVALID, (b"excl_ptr decreases", b"batch position 1"))
    edited(eidx, 1, -1, _lib.RWR_E_RANGE, (b"exclusion index", b"batch position 2"))
    for d in (-0.25, 1.5, float("nan")):
        st, msg = call(d=d)
        assert st == _lib.RWR_E_UNSUPPORTED and b"[0, 1]" in msg and untouched(), d
    # a correct call afterwards answers right
    restarts = [(idx[0:2], val[0:2]), (idx[2:3], val[2:3]), (idx[3:5], val[3:5])]
    sets = [eidx[0:1], eidx[1:1], eidx[1:3]]
    w = Case(amd, c.g, restarts, start, sets)
    assert call()[0] == _lib.RWR_OK and not untouched()
    _check((ids, sc, cnt), w.want([0, 1, 2], 3, top_n, gg.NODE_USER, FOLLOWS, True, True), "after the refusals")
    w.close()
