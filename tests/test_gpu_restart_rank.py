"""Restart-vector walks ranked on the device (rwr_recommend_restart_batch / Recommender.RecommendationRestartBatch, DESIGN
§3.12).  The expectation is always the composition the header states, built from verified pieces: the row rwr_model_run_restart
returns for the vector, the candidates (ITEM nodes that no member of the exclusion set LIKEs) and their order (score
descending, then id descending) in NumPy as tests/rank_reference.py does for one seed.  Ids must be equal, scores bitwise equal.

Graphs: ~5 000 items (more than the select kernels' 4 096 candidate slots: radix select below top-1024, radix sort above) and
~600 items (the one-workgroup sort), a weighted one, one with dangling users in supports and sets, one whose hub user's raw
list spans two exclusion segments.  Batches of 2, 19 and 70 vectors at tile widths 1-64 with one tile per tile group (several
groups, padding slots), 0, 1 and 10 steps, top-1 to more than there are items."""
import ctypes as C

import numpy as np
import pytest

from tests import graphgen as gg

pytestmark = pytest.mark.gpu

EXACT_MAX = 256
D = 0.15
PI64, PI32, PD = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_double)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def amd():
    import recommendersystems_amd as m
    from recommendersystems_amd import _lib
    assert _lib.load().rwr_device_count() >= 1, "no gfx950 device: the HIP path cannot run"
    return m


def _single_row(G, n, idx, val, start, d, T):
    """the rank row of rwr_model_run_restart for one vector after T steps"""
    from recommendersystems_amd import _lib
    lib = _lib.load()
    v = np.zeros(n)
    v[np.asarray(idx, dtype=np.int64)] = val
    x = np.ones(n) if start < 0 else np.zeros(n)
    if start >= 0:
        x[start] = float(n)
    out = np.empty(n)
    st = lib.rwr_model_run_restart(G._handle(), v.ctypes.data_as(PD), x.ctypes.data_as(PD), d, _lib.RWR_RUN_ITERATIONS,
                                   float(max(T, 0)), out.ctypes.data_as(PD), None)
    assert st == _lib.RWR_OK, lib.rwr_last_error()
    return out


def _liked(g, members):
    """rows that some member's RAW list holds with type LIKE (Recommender.cs:20-24 for every member)"""
    out = []
    for m in members:
        lo, hi = int(g["rowptr"][m]), int(g["rowptr"][m + 1])
        out.append(g["dst"][lo:hi][g["etype"][lo:hi] == gg.EDGE_LIKE].astype(np.int64))
    return np.concatenate(out) if out else np.zeros(0, dtype=np.int64)


def _ranked(g, row, members):
    """the whole ranked list of one rank row: (ids, scores), tests/rank_reference.py's order over a set of excluded nodes"""
    cand = g["node_type"] == gg.NODE_ITEM
    cand[_liked(g, members)] = False
    rows = np.flatnonzero(cand)
    s, ids = row[rows], g["node_id"][rows]
    order = np.lexsort((ids, s))[::-1]
    return ids[order], s[order]


def _packed(lists, top_n):
    K = len(lists)
    ids, sc, cnt = np.zeros((K, top_n), dtype=np.int64), np.zeros((K, top_n)), np.zeros(K, dtype=np.int32)
    for k, (i, s) in enumerate(lists):
        c = min(top_n, len(i))
        ids[k, :c], sc[k, :c], cnt[k] = i[:c], s[:c], c
    return ids, sc, cnt


def _check(got, want, what):
    ids, sc, cnt = got
    wi, ws, wc = want
    assert (cnt == wc).all(), (what, "counts", cnt.tolist(), wc.tolist())
    bad = np.flatnonzero((ids != wi).any(axis=1))
    assert bad.size == 0, (what, "ids differ in rows", bad.tolist())
    bad = np.flatnonzero((bits(sc) != bits(ws)).any(axis=1))
    assert bad.size == 0, (what, "scores not bitwise equal in rows", bad.tolist())


def _vectors(g, n_users, K, rng):
    """K non-negative vectors over users and a few items, of 0 to 64 entries, some entries +-0.0; starts of every kind"""
    n = len(g["node_id"])
    sizes = [8, 1, 0, 3, 8, 64, 2, 8, 1, 5, 8, 8, 16, 1, 4, 8, 2, 8, 8, 3, 1]
    restarts = []
    for k in range(K):
        m = sizes[k % len(sizes)]
        idx = rng.choice(n_users, m, replace=False).astype(np.int32)
        if m >= 3 and k % 3 == 0:
            idx[1] = n_users + int(rng.integers(0, n - n_users))  # an ITEM (or ETC) node in the support
        val = rng.random(m) + 0.05
        if m >= 2 and k % 5 == 1:
            val[0] = 0.0 if k % 2 else -0.0                       # dropped from the walk, still a member of the default set
        restarts.append((idx, val))
    starts = rng.integers(-1, n, K).astype(np.int32)
    starts[::4] = -1
    return restarts, starts


def _sets(restarts, n_users, rng):
    """explicit exclusion sets, different from the supports: empty, a member twice, several users, an item among them"""
    sets = []
    for k in range(len(restarts)):
        users = rng.choice(n_users, 3, replace=False).astype(np.int32)
        if k % 4 == 0:
            sets.append(np.zeros(0, dtype=np.int32))
        elif k % 4 == 1:
            sets.append(np.array([users[0], users[1], users[0]], dtype=np.int32))
        elif k % 4 == 2:
            sets.append(np.array([0, 1, users[2]], dtype=np.int32))   # the two most active users: they share liked items
        else:
            sets.append(np.array([users[0], n_users + int(users[1])], dtype=np.int32))
    return sets


class Case:
    """a graph, 70 vectors, two families of exclusion sets, and the single calls' rows and whole ranked lists per step count"""

    def __init__(self, amd, g, n_users, seed):
        self.amd, self.g, self.n_users = amd, g, n_users
        self.n = len(g["node_id"])
        self.n_items = int((g["node_type"] == gg.NODE_ITEM).sum())
        rng = np.random.default_rng(seed)
        self.restarts, self.starts = _vectors(g, n_users, 70, rng)
        self.sets = _sets(self.restarts, n_users, rng)
        self.G = amd.Graph.from_flat(**g)
        self.G.buildGraph()
        self._rows, self._lists = {}, {}

    def close(self):
        self.G.close()

    def members(self, k, explicit):
        return self.sets[k] if explicit else self.restarts[k][0]

    def row(self, k, T):
        if (k, T) not in self._rows:
            idx, val = self.restarts[k]
            self._rows[(k, T)] = _single_row(self.G, self.n, idx, val, int(self.starts[k]), D, T)
        return self._rows[(k, T)]

    def ranked(self, k, T, explicit):
        key = (k, T, explicit)
        if key not in self._lists:
            self._lists[key] = _ranked(self.g, self.row(k, T), self.members(k, explicit))
        return self._lists[key]

    def want(self, K, T, top_n, explicit):
        return _packed([self.ranked(k, T, explicit) for k in range(K)], top_n)

    def call(self, H, K, T, top_n, explicit):
        rec = self.amd.Recommender(H)
        return rec.RecommendationRestartBatch(self.restarts[:K], self.starts[:K], D, T, top_n,
                                              exclude=self.sets[:K] if explicit else None)

    def sweep(self, tile_seeds, Ks=(2, 19, 70), Ts=(0, 1, 10), tops=None):
        tops = tops or (1, 100, 1024, 1025, self.n_items + 5)
        H = self.amd.Graph.from_flat(**self.g, tile_seeds=tile_seeds, tile_group=1)
        H.buildGraph()
        try:
            for K in Ks:
                for ti, T in enumerate(Ts):
                    for pi, top_n in enumerate(tops):
                        explicit = (ti + pi + K) % 2 == 1           # both families at every K, step count and width
                        got = self.call(H, K, T, top_n, explicit)
                        _check(got, self.want(K, T, top_n, explicit), (tile_seeds, K, T, top_n, explicit))
                        if top_n > self.n_items:                    # fewer candidates than top_n: a zero-filled tail
                            ids, sc, cnt = got
                            assert (cnt < top_n).all() and (cnt > 0).any()
                            for k in range(K):
                                assert not ids[k, cnt[k]:].any() and not bits(sc[k, cnt[k]:]).any()
        finally:
            H.close()


@pytest.fixture(scope="module")
def big(amd):
    """~300 users, 5 000 items: more items than SEL_SLOTS = 4096"""
    g = gg.random_graph(31, n_users=300, n_items=5000, n_likes=9000, n_etc=6, n_friend=250, n_mention=120, n_author=60)
    c = Case(amd, g, 300, 5)
    assert c.n_items > 4096
    yield c
    c.close()


@pytest.fixture(scope="module")
def small(amd):
    """~200 users, 600 items: the one-workgroup ranking"""
    g = gg.random_graph(32, n_users=200, n_items=600, n_likes=3000, n_etc=4, n_friend=150, n_mention=80, n_author=40)
    c = Case(amd, g, 200, 6)
    yield c
    c.close()


def test_the_cases_hold_what_they_claim(big):
    """two members of one set like the same item, a set lists a member twice, a set is empty, a default set has a member
    whose value is zero"""
    c = big
    shared = [k for k in range(70) if len(c.sets[k]) and len(np.unique(_liked(c.g, c.sets[k]))) < len(_liked(c.g, np.unique(c.sets[k])))]
    assert shared, "no explicit set whose members like a common item"
    assert any(len(s) != len(np.unique(s)) for s in c.sets) and any(len(s) == 0 for s in c.sets)
    assert any((v == 0.0).any() for _, v in c.restarts[:19])
    assert any(len(i) == 0 for i, _ in c.restarts[:19])
    # the sets differ from the supports, and so do the lists
    k = 5
    assert set(c.sets[k].tolist()) != set(c.restarts[k][0].tolist())
    assert not np.array_equal(c.ranked(k, 10, True)[0][:100], c.ranked(k, 10, False)[0][:100])


@pytest.mark.parametrize("tile_seeds", [1, 4, 16, 64])
def test_big_graph_every_width(big, tile_seeds):
    big.sweep(tile_seeds)


@pytest.mark.parametrize("tile_seeds", [1, 4, 16, 64])
def test_small_graph_every_width(small, tile_seeds):
    small.sweep(tile_seeds)


def test_default_opts_on_the_reference_handle(big):
    """the handle the single calls ran on, with the library's own tile width and tile group"""
    c = big
    for K, T, top_n, explicit in ((70, 10, 100, False), (19, 1, 1025, True), (2, 0, 1, False)):
        _check(c.call(c.G, K, T, top_n, explicit), c.want(K, T, top_n, explicit), (K, T, top_n, explicit))
    # a negative count runs no step, as rwr_recommend_batch treats it
    _check(c.call(c.G, 19, -3, 100, True), c.want(19, 0, 100, True), "n_iter < 0")


def test_weighted_graph(amd):
    """non-uniform weights (MENTION links): the weighted kernels' own values"""
    g = gg.random_graph(33, n_users=250, n_items=700, n_likes=3500, n_etc=8, n_friend=300, n_mention=900, n_author=80)
    assert len(np.unique(g["w"])) > 10
    c = Case(amd, g, 250, 7)
    try:
        c.sweep(16, Ks=(19,), Ts=(1, 10), tops=(100, 1025))
        c.sweep(0, Ks=(70,), Ts=(10,), tops=(100,))
    finally:
        c.close()


def test_dangling_users_in_supports_and_sets(amd):
    g = gg.random_graph(34, n_users=400, n_items=600, n_likes=1500, n_friend=40)
    n = len(g["node_id"])
    deg = np.diff(g["rowptr"])
    dang = np.flatnonzero(deg[:400] == 0).astype(np.int32)
    assert len(dang) >= 4
    c = Case(amd, g, 400, 8)
    try:
        c.restarts[0] = (np.array([dang[0], 3, dang[1]], dtype=np.int32), np.array([0.5, 0.25, 0.25]))
        c.restarts[1] = (np.array([dang[2]], dtype=np.int32), np.array([1.0]))      # all of the mass returns to a dangling node
        c.starts[1] = dang[2]
        c.starts[2] = dang[3]
        c.sets[1] = np.array([dang[0], dang[1]], dtype=np.int32)                    # members without raw links: no segment
        c.sets[2] = np.array([dang[0], 0], dtype=np.int32)
        c.sweep(4, Ks=(19,), Ts=(0, 1, 10), tops=(100, n))
    finally:
        c.close()


def _with_hub(g, n_users, hub, n_new):
    """user `hub` also LIKEs the first n_new items it does not like yet: its raw list grows past one segment"""
    lo, hi = int(g["rowptr"][hub]), int(g["rowptr"][hub + 1])
    have = set(g["dst"][lo:hi][g["etype"][lo:hi] == gg.EDGE_LIKE].tolist())
    items = np.flatnonzero(g["node_type"] == gg.NODE_ITEM)
    new = np.array([i for i in items if i not in have][:n_new], dtype=np.int32)
    ins = lambda a, v: np.concatenate([a[:hi], v, a[hi:]])
    rowptr = g["rowptr"].copy()
    rowptr[hub + 1:] += len(new)
    return dict(g, rowptr=rowptr, dst=ins(g["dst"], new), etype=ins(g["etype"], np.full(len(new), gg.EDGE_LIKE, dtype=np.uint8)),
                w=ins(g["w"], np.ones(len(new))))


def test_hub_user_spans_two_segments(amd):
    g0 = gg.random_graph(35, n_users=120, n_items=5200, n_likes=4000, n_friend=60)
    g = _with_hub(g0, 120, 7, 4300)
    assert 4096 < int(g["rowptr"][8] - g["rowptr"][7]) <= 8192
    c = Case(amd, g, 120, 9)
    try:
        c.restarts[0] = (np.array([7, 11], dtype=np.int32), np.array([0.5, 0.5]))   # the hub in a support (the default set)
        c.sets[1] = np.array([30, 7, 31], dtype=np.int32)                           # ... and between two others in a set
        c.sets[2] = np.array([7, 7], dtype=np.int32)
        for explicit in (False, True):
            assert c.n_items - len(np.unique(_liked(g, c.members(0 if not explicit else 1, explicit)))) < 1024
        H = amd.Graph.from_flat(**g, tile_seeds=4, tile_group=1)
        H.buildGraph()
        for T, top_n, explicit in ((10, 100, False), (10, 100, True), (1, 1024, True), (1, 1025, False), (0, c.n_items + 5, True)):
            _check(c.call(H, 19, T, top_n, explicit), c.want(19, T, top_n, explicit), ("hub", T, top_n, explicit))
        H.close()
    finally:
        c.close()


class OddTypes:
    """A graph of 30 nodes whose user `u` has exactly five raw links, of types LIKE, 2, 7, 8 and 255, to five different items
    (the exclusion's mask has a bit for 1, 2 and 7, none for 8 and 255); three vectors with u in the sets of the first and the
    last; their rows from rwr_model_run_restart_batch on a handle of tile width 2: two tiles, one padding slot."""
    TYPES = (gg.EDGE_LIKE, 2, 7, 8, 255)
    T = 4

    def __init__(self, amd):
        g = gg.random_graph(36, n_users=10, n_items=20, n_likes=70, uniform=True)
        deg = np.diff(g["rowptr"])
        u = next(i for i in range(10) if deg[i] >= 5)
        lo, hi = int(g["rowptr"][u]), int(g["rowptr"][u + 1])
        keep = np.r_[0:lo + 5, hi:len(g["dst"])]                    # u keeps its first five links
        rowptr = g["rowptr"].copy()
        rowptr[u + 1:] -= hi - (lo + 5)
        etype = g["etype"][keep].copy()
        etype[lo:lo + 5] = self.TYPES
        self.g = dict(g, rowptr=rowptr, dst=g["dst"][keep], etype=etype, w=g["w"][keep])
        self.u, self.targets = u, self.g["dst"][lo:lo + 5].astype(np.int64)
        assert len(set(self.targets.tolist())) == 5 and (self.g["node_type"][self.targets] == gg.NODE_ITEM).all()
        self.n_items = 20
        # a second user with links, none of them to u's five items: its set membership hides none of them
        v = next(i for i in range(10) if i != u and deg[i] > 0 and not np.isin(_liked(self.g, [i]), self.targets).any())
        self.restarts = [{u: 1.0}, {v: 1.0}, {u: 0.5, v: 0.5}]
        self.starts = np.array([u, -1, v], dtype=np.int32)
        self.sets = [np.array([u], dtype=np.int32), np.zeros(0, dtype=np.int32), np.array([v, u], dtype=np.int32)]
        self.H = amd.Graph.from_flat(**self.g, tile_seeds=2, tile_group=1)
        self.H.buildGraph()
        self.rows, _ = amd.Model.RunRestartBatch(self.H, D, self.restarts, self.starts, self.T)
        self.lists = [_ranked(self.g, self.rows[k], self.sets[k]) for k in range(3)]

    def close(self):
        self.H.close()


def test_unnamed_link_types_are_not_excluded(amd):
    """the untyped end runs the typed exclusion kernel with the mask 1 << LIKE: of a member's links of types LIKE, 2, 7, 8 and
    255 only the LIKE target leaves the list (8 and 255 have no bit in the mask: a shift by them must not happen)"""
    c = OddTypes(amd)
    try:
        ids_of = c.g["node_id"][c.targets]
        for top_n in (c.n_items + 5, 1025):                         # the select and the sort
            ids, sc, cnt = amd.Recommender(c.H).RecommendationRestartBatch(c.restarts, c.starts, D, c.T, top_n, exclude=c.sets)
            _check((ids, sc, cnt), _packed(c.lists, top_n), ("odd types", top_n))
            assert cnt.tolist() == [c.n_items - 1, c.n_items, len(c.lists[2][0])]
            for k in (0, 2):
                got = dict(zip(ids[k, :cnt[k]].tolist(), bits(sc[k, :cnt[k]]).tolist()))
                assert int(ids_of[0]) not in got, (k, "the LIKE target is in the list")
                for t, i in zip(c.targets[1:], ids_of[1:]):
                    assert got.get(int(i)) == int(bits(c.rows[k, t:t + 1])[0]), (k, int(t))
            assert set(ids_of.tolist()) <= set(ids[1, :cnt[1]].tolist())   # the set without u excludes none of them
    finally:
        c.close()


def test_against_the_python_oracle(small):
    """the literal oracle's Model with the sparse-restart idiom of tests/test_gpu_restart_batch.py, and a Python sort"""
    from tests.test_gpu_restart_batch import _oracle_graph, _oracle_model
    c = small
    PG = _oracle_graph(c.g)
    K, T, top_n = 6, 10, 100
    got = c.call(c.G, K, T, top_n, True)
    for k in range(K):
        idx, val = c.restarts[k]
        m = _oracle_model(PG, D, int(c.starts[k]), idx, val)
        for _ in range(T):
            m.deliverRanks(); m.updateRanks()
        liked = set(_liked(c.g, c.sets[k]).tolist())
        cand = [(float(m.rank[i]), int(c.g["node_id"][i])) for i in range(c.n)
                if c.g["node_type"][i] == gg.NODE_ITEM and i not in liked]
        cand.sort(key=lambda e: (-e[0], -e[1]))
        cand = cand[:top_n]
        assert got[2][k] == len(cand)
        assert got[0][k, :len(cand)].tolist() == [e[1] for e in cand], k
        assert (bits(got[1][k, :len(cand)]) == bits(np.array([e[0] for e in cand]))).all(), k


def test_reduces_to_the_single_seed_recommendation(amd, big):
    """{s: 1.0} with start = s and exclusion {s} at d = (double)(float)0.15 is Recommendation(s): rwr_recommend_batch's ids
    and score bits, for seeds that are not dangling (those it answers without iterating)"""
    c = big
    deg = np.diff(c.g["rowptr"])
    seeds = np.array([s for s in (0, 1, 5, 17, 40, 133, 250, 299, 305, 4000) if deg[s] > 0], dtype=np.int32)
    assert len(seeds) >= 6
    d = float(np.float32(0.15))
    rec = amd.Recommender(c.G)
    for T, top_n in ((10, 100), (3, 1025)):
        want = rec.RecommendationBatch(seeds, 0.15, T, top_n)
        got = rec.RecommendationRestartBatch([{int(s): 1.0} for s in seeds], seeds, d, T, top_n, exclude=[[int(s)] for s in seeds])
        _check(got, want, ("single seeds", T, top_n))
        got = rec.RecommendationRestartBatch([{int(s): 1.0} for s in seeds], seeds, d, T, top_n)    # the default sets
        _check(got, want, ("single seeds, default sets", T, top_n))


def test_fallbacks_rank_the_single_calls_rows(amd, big):
    """K = 1, and a vector of 300 entries (the tolerance class) inside a batch: vector by vector through rwr_model_run_restart"""
    c = big
    rng = np.random.default_rng(23)
    wide = (rng.choice(c.n, 300, replace=False).astype(np.int32), rng.random(300) + 1e-3)
    assert len(wide[0]) > EXACT_MAX
    rs = [c.restarts[3], wide, c.restarts[4], c.restarts[1]]
    st = np.array([-1, 2, 9, -1], dtype=np.int32)
    sets = [c.sets[1], wide[0][:5], np.zeros(0, dtype=np.int32), c.sets[2]]
    rec = amd.Recommender(c.G)
    for T, top_n in ((4, 100), (4, 1025)):
        rows = [_single_row(c.G, c.n, i, v, int(s), D, T) for (i, v), s in zip(rs, st)]
        for explicit in (True, False):
            members = sets if explicit else [i for i, _ in rs]
            want = _packed([_ranked(c.g, r, m) for r, m in zip(rows, members)], top_n)
            _check(rec.RecommendationRestartBatch(rs, st, D, T, top_n, exclude=sets if explicit else None), want, ("wide", T, top_n))
        for k in (0, 1):                                                            # one vector
            want = _packed([_ranked(c.g, rows[k], sets[k])], top_n)
            _check(rec.RecommendationRestartBatch([rs[k]], st[k:k + 1], D, T, top_n, exclude=[sets[k]]), want, ("K=1", k, T, top_n))


def test_handle_reuse_in_both_directions(amd, small):
    """this call leaves -1 markers in X: a later call of any entry on the handle must not see them, and this call must not
    see what the others leave"""
    c = small
    g = c.g
    seeds = np.random.default_rng(4).integers(0, c.n, 40).astype(np.int32)

    def ranked(H):
        return c.call(H, 19, 5, 100, True)

    def full(H):
        return amd.Model.RunRestartBatch(H, D, c.restarts[:19], c.starts[:19], 5)

    def single_seeds(H):
        return amd.Recommender(H).RecommendationBatch(seeds, 0.15, 10, 20)

    def fresh(f):
        H = amd.Graph.from_flat(**g, tile_seeds=16)
        H.buildGraph()
        try:
            return f(H)
        finally:
            H.close()

    want = {f: fresh(f) for f in (ranked, full, single_seeds)}
    _check(want[ranked], c.want(19, 5, 100, True), "fresh handle")
    for first, second in ((ranked, full), (ranked, single_seeds), (full, ranked), (single_seeds, ranked), (ranked, ranked)):
        H = amd.Graph.from_flat(**g, tile_seeds=16)
        H.buildGraph()
        first(H)
        got = second(H)
        H.close()
        for a, b in zip(got, want[second]):
            if a.dtype == np.float64:
                assert (bits(a) == bits(b)).all(), (first.__name__, second.__name__)
            else:
                assert (a == b).all(), (first.__name__, second.__name__)


def test_errors_on_a_live_graph(amd, small):
    from recommendersystems_amd import _lib
    c = small
    n, G = c.n, c.G
    rec = amd.Recommender(G)
    ok = [({1: 0.5, 7: 0.25}), ({3: 1.0}), ({4: 2.0, 9: 1.0, 11: 0.5})]

    def still_right():
        _check(c.call(G, 19, 1, 100, True), c.want(19, 1, 100, True), "after a refused call")

    def refused(status, *words, restarts=ok, starts=None, d=D, T=3, top_n=10, exclude=None):
        with pytest.raises(amd.RwrError) as ei:
            rec.RecommendationRestartBatch(restarts, starts, d, T, top_n, exclude=exclude)
        assert ei.value.status == status, str(ei.value)
        for w in ("rwr_recommend_restart_batch",) + words:
            assert w in str(ei.value), (w, str(ei.value))

    # what rwr_model_run_restart_batch reports for the vectors, with the same status and the batch position
    refused(_lib.RWR_E_INVALID, "index 4", "vector 1", restarts=[ok[0], ([4, 9, 4], [1.0, 2.0, 3.0]), ok[2]])
    refused(_lib.RWR_E_RANGE, "batch position 2", restarts=[ok[0], ok[1], ([4, n], [1.0, 2.0])])
    refused(_lib.RWR_E_RANGE, "batch position 1", starts=[0, n, -1])
    refused(_lib.RWR_E_RANGE, "batch position 2", starts=[0, 1, -2])
    for bad in (np.inf, -np.inf, np.nan):
        refused(_lib.RWR_E_UNSUPPORTED, "restart", "batch position 1", restarts=[ok[0], ([4, 9], [0.5, bad])])
    still_right()
    # the domain of the Recommendation entries
    refused(_lib.RWR_E_UNSUPPORTED, "negative", "batch position 2", restarts=[ok[0], ok[1], ([4, 9], [0.5, -1e-300])])
    for d in (-0.01, 1.5, np.nan):
        refused(_lib.RWR_E_UNSUPPORTED, "damping factor", d=d)
    refused(_lib.RWR_E_INVALID, "top_n", top_n=0)
    refused(_lib.RWR_E_INVALID, "top_n", top_n=-4)
    # the exclusion sets
    refused(_lib.RWR_E_RANGE, "exclusion index %d" % n, "batch position 1", exclude=[[1], [2, n], [3]])
    refused(_lib.RWR_E_RANGE, "exclusion index -1", "batch position 2", exclude=[[1], [], [3, -1]])
    still_right()
    gb = gg.random_graph(5, n_users=50, n_items=120, n_likes=700, n_friend=60, n_mention=50)
    w = gb["w"].copy()
    pick = np.random.default_rng(3).choice(len(w), 40, replace=False)
    w[pick] = -0.25 * w[pick]
    H = amd.Graph.from_flat(**dict(gb, w=w))
    H.buildGraph()
    with pytest.raises(amd.RwrError) as ei:
        amd.Recommender(H).RecommendationRestartBatch(ok, None, D, 3, 10)
    assert ei.value.status == _lib.RWR_E_UNSUPPORTED and "non-negative" in str(ei.value)
    amd.Model.RunRestartBatch(H, D, ok, None, 3)                   # the full-vector call remains the way
    H.close()

    # the raw entry: pointers, K, and that a refused call writes nothing
    lib = _lib.load()
    ptr, idx, val = np.array([0, 1, 2], dtype=np.int64), np.array([1, 2], dtype=np.int32), np.array([1.0, 1.0])
    ids, sc, cnt = np.full((2, 10), 7, dtype=np.int64), np.full((2, 10), 7.0), np.full(2, -5, dtype=np.int32)
    ep, ei_ = np.array([0, 1, 2], dtype=np.int64), np.array([5, 6], dtype=np.int32)
    pp, pi, pv = ptr.ctypes.data_as(PI64), idx.ctypes.data_as(PI32), val.ctypes.data_as(PD)
    pids, psc, pcnt = ids.ctypes.data_as(PI64), sc.ctypes.data_as(PD), cnt.ctypes.data_as(PI32)
    pep, pei = ep.ctypes.data_as(PI64), ei_.ctypes.data_as(PI32)
    h, call = G._handle(), lib.rwr_recommend_restart_batch
    assert call(h, -1, pp, pi, pv, None, pep, pei, D, 3, 10, pids, psc, pcnt) == _lib.RWR_E_INVALID
    assert b"negative K" in lib.rwr_last_error()
    assert call(h, 0, None, None, None, None, None, None, D, 3, 10, None, None, None) == _lib.RWR_OK
    assert call(h, 2, None, pi, pv, None, pep, pei, D, 3, 10, pids, psc, pcnt) == _lib.RWR_E_INVALID
    assert call(h, 2, pp, None, pv, None, pep, pei, D, 3, 10, pids, psc, pcnt) == _lib.RWR_E_INVALID
    assert call(h, 2, pp, pi, None, None, pep, pei, D, 3, 10, pids, psc, pcnt) == _lib.RWR_E_INVALID
    for outs in ((None, psc, pcnt), (pids, None, pcnt), (pids, psc, None)):
        assert call(h, 2, pp, pi, pv, None, pep, pei, D, 3, 10, *outs) == _lib.RWR_E_INVALID
        assert b"rwr_recommend_restart_batch" in lib.rwr_last_error()
    for bad_ptr in ([1, 1, 2], [0, 2, 1]):
        bp = np.array(bad_ptr, dtype=np.int64)
        assert call(h, 2, bp.ctypes.data_as(PI64), pi, pv, None, pep, pei, D, 3, 10, pids, psc, pcnt) == _lib.RWR_E_INVALID
        assert b"sup_ptr" in lib.rwr_last_error()
        assert call(h, 2, pp, pi, pv, None, bp.ctypes.data_as(PI64), pei, D, 3, 10, pids, psc, pcnt) == _lib.RWR_E_INVALID
        assert b"excl_ptr" in lib.rwr_last_error()
    assert call(h, 2, pp, pi, pv, None, pep, None, D, 3, 10, pids, psc, pcnt) == _lib.RWR_E_INVALID
    assert b"excl_idx" in lib.rwr_last_error()
    assert (ids == 7).all() and (sc == 7.0).all() and (cnt == -5).all(), "a refused call wrote results"
    # empty sets with a NULL index array, empty supports with NULL index and value arrays: link-only walks, nothing excluded
    zp = np.zeros(3, dtype=np.int64)
    pz = zp.ctypes.data_as(PI64)
    assert call(h, 2, pz, None, None, None, pz, None, D, 3, 10, pids, psc, pcnt) == _lib.RWR_OK
    want = rec.RecommendationRestartBatch([{}, {}], None, D, 3, 10, exclude=[[], []])
    _check((ids, sc, cnt), want, "NULL arrays")
    row = _single_row(G, n, [], [], -1, D, 3)
    _check(want, _packed([_ranked(c.g, row, [])] * 2, 10), "link-only walks")
    # K = 0 through the mirror
    e = rec.RecommendationRestartBatch([], None, D, 3, 10)
    assert e[0].shape == (0, 10) and e[2].shape == (0,)
    still_right()
