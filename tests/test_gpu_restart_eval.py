"""Restart-vector walks evaluated on the device (rwr_recommend_restart_eval_batch /
Recommender.RecommendationRestartEvalBatch).  The expectation is the composition the header states, built as
tests/test_gpu_restart_rank.py builds its lists: the row rwr_model_run_restart returns for the vector, the candidates and their
order in NumPy over the exclusion set, then oracle.rwr_oracle.evaluate (Experiment.cs:121-128) on the id list, cut to top_n
when top_n > 0.  The integers must be equal, sum_precision bitwise equal.

Graphs as in that file: ~5 000 items (hit lists longer than the one-workgroup sort's 4 096 keys when a test set names every
item: the radix sort and the global counters) and ~600 items, a weighted one, one with dangling users, one with a hub user."""
import ctypes as C

import numpy as np
import pytest

from oracle.rwr_oracle import evaluate
from tests import graphgen as gg
from tests.test_gpu_restart_rank import D, EXACT_MAX, Case, OddTypes, _liked, _ranked, _single_row, _with_hub, bits

pytestmark = pytest.mark.gpu

PI64, PI32, PD = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_double)
N_FAMILIES = 9


@pytest.fixture(scope="module")
def amd():
    import recommendersystems_amd as m
    from recommendersystems_amd import _lib
    assert _lib.load().rwr_device_count() >= 1, "no gfx950 device: the HIP path cannot run"
    return m


def _want(ids, test, top_n):
    """(nHits, sumPrecision, len) of the whole ranked id list, cut to top_n when top_n > 0"""
    ids = ids[:top_n] if top_n > 0 else ids
    h, sp = evaluate([(int(i),) for i in ids], set(int(t) for t in test))
    return h, sp, len(ids)


def _check(got, want, what):
    hits, sp, ln = got
    wh = np.array([w[0] for w in want], dtype=np.int64)
    ws = np.array([w[1] for w in want], dtype=np.float64)
    wl = np.array([w[2] for w in want], dtype=np.int64)
    assert (ln == wl).all(), (what, "list_len", ln.tolist(), wl.tolist())
    assert (hits == wh).all(), (what, "n_hits", hits.tolist(), wh.tolist())
    bad = np.flatnonzero(bits(sp) != bits(ws))
    assert bad.size == 0, (what, "sum_precision not bitwise equal at", bad.tolist(), sp[bad].tolist(), ws[bad].tolist())


class EvalCase(Case):
    """Case with one test set per vector, of a family chosen by (k + shift) % 9"""

    def __init__(self, amd, g, n_users, seed):
        super().__init__(amd, g, n_users, seed)
        self.item_rows = np.flatnonzero(g["node_type"] == gg.NODE_ITEM)
        self.item_ids = g["node_id"][self.item_rows]
        self.other_ids = g["node_id"][g["node_type"] != gg.NODE_ITEM]
        self.rng_seed = seed
        self._want = {}

    def test_set(self, k, T, explicit, shift):
        fam = (k + shift) % N_FAMILIES
        rng = np.random.default_rng(self.rng_seed * 1000 + k)
        ids, _ = self.ranked(k, T, explicit)
        held = rng.choice(self.item_ids, 40, replace=False)
        if fam == 0:
            return np.zeros(0, dtype=np.int64)
        if fam == 1:                                                # ids no node has (graphgen's ids are 1000 + 7 i)
            return np.array([1, -5, 1001, 2 ** 40, -2 ** 62], dtype=np.int64)
        if fam == 2:                                                # excluded items must not count; three that do
            liked = np.unique(_liked(self.g, self.members(k, explicit)))
            return np.concatenate([self.g["node_id"][liked], held[:3]])
        if fam == 3:                                                # users and ETC nodes are no candidates
            return np.concatenate([rng.choice(self.other_ids, 20, replace=False), held[:2]])
        if fam == 4:                                                # duplicates change nothing
            return np.concatenate([held[:10], held[:10], held[:5], held[:1]])
        if fam == 5:                                                # the realistic case: a few dozen held-out likes
            return held
        if fam == 6:                                                # every item: the longest hit list there is
            return rng.permutation(self.item_ids)
        if fam == 7:
            return ids[:1].copy()                                   # the only hit is the first-ranked candidate
        return ids[-1:].copy()                                      # ... the last-ranked

    def tests(self, K, T, explicit, shift):
        return [self.test_set(k, T, explicit, shift) for k in range(K)]

    def want_eval(self, K, T, top_n, explicit, shift):
        out = []
        for k in range(K):
            key = (k, T, top_n, explicit, shift % N_FAMILIES)
            if key not in self._want:
                self._want[key] = _want(self.ranked(k, T, explicit)[0], self.test_set(k, T, explicit, shift), top_n)
            out.append(self._want[key])
        return out

    def call_eval(self, H, K, T, top_n, explicit, shift):
        rec = self.amd.Recommender(H)
        return rec.RecommendationRestartEvalBatch(self.restarts[:K], self.starts[:K], D, T, self.tests(K, T, explicit, shift),
                                                  topN=top_n, exclude=self.sets[:K] if explicit else None)

    def sweep_eval(self, tile_seeds, Ks=(2, 19, 70), Ts=(0, 1, 10), tops=None):
        tops = tops if tops is not None else (0, 1, 100, self.n_items + 5)
        H = self.amd.Graph.from_flat(**self.g, tile_seeds=tile_seeds, tile_group=1)
        H.buildGraph()
        try:
            for K in Ks:
                for ti, T in enumerate(Ts):
                    for pi, top_n in enumerate(tops):
                        explicit = (ti + pi + K) % 2 == 1
                        shift = 3 * ti + pi + (0 if K > 2 else 2 * ti)   # every family reaches every K, step count and width
                        got = self.call_eval(H, K, T, top_n, explicit, shift)
                        _check(got, self.want_eval(K, T, top_n, explicit, shift), (tile_seeds, K, T, top_n, explicit, shift))
        finally:
            H.close()


@pytest.fixture(scope="module")
def big(amd):
    g = gg.random_graph(31, n_users=300, n_items=5000, n_likes=9000, n_etc=6, n_friend=250, n_mention=120, n_author=60)
    c = EvalCase(amd, g, 300, 5)
    assert c.n_items > 4096
    yield c
    c.close()


@pytest.fixture(scope="module")
def small(amd):
    g = gg.random_graph(32, n_users=200, n_items=600, n_likes=3000, n_etc=4, n_friend=150, n_mention=80, n_author=40)
    c = EvalCase(amd, g, 200, 6)
    yield c
    c.close()


def test_the_cases_hold_what_they_claim(big):
    c = big
    fams = {(k + 0) % N_FAMILIES: c.test_set(k, 10, True, 0) for k in range(N_FAMILIES)}
    assert len(fams[0]) == 0
    assert not np.isin(fams[1], c.g["node_id"]).any()
    assert len(fams[6]) > 4096 and len(np.unique(fams[4])) < len(fams[4])
    # family 2 names excluded items that would be hits otherwise; the expectation counts only the three others at most
    k = 2
    liked = np.unique(_liked(c.g, c.members(k, True)))
    assert len(liked) > 0 and _want(c.ranked(k, 10, True)[0], fams[2], 0)[0] <= 3
    assert _want(c.ranked(3, 10, True)[0], fams[3], 0)[0] <= 2
    h7, sp7, _ = _want(c.ranked(7, 10, True)[0], fams[7], 0)
    assert (h7, sp7) == (1, 1.0)
    h8, sp8, n8 = _want(c.ranked(8, 10, True)[0], fams[8], 0)
    assert h8 == 1 and sp8 == 1.0 / n8
    # after 0 steps from rank 1 everywhere every score is equal: the order is the ids' alone
    k0 = int(np.flatnonzero(c.starts[:19] < 0)[0])
    assert len(np.unique(c.ranked(k0, 0, False)[1])) == 1


@pytest.mark.parametrize("tile_seeds", [1, 4, 16, 64])
def test_big_graph_every_width(big, tile_seeds):
    big.sweep_eval(tile_seeds)


@pytest.mark.parametrize("tile_seeds", [1, 4, 16, 64])
def test_small_graph_every_width(small, tile_seeds):
    small.sweep_eval(tile_seeds)


def test_default_opts_on_the_reference_handle(big):
    c = big
    for K, T, top_n, explicit, shift in ((70, 10, 0, False, 0), (19, 1, 100, True, 4), (2, 0, 1, False, 5)):
        _check(c.call_eval(c.G, K, T, top_n, explicit, shift), c.want_eval(K, T, top_n, explicit, shift), (K, T, top_n, explicit))
    # a negative count runs no step; a negative top_n keeps the whole list
    _check(c.call_eval(c.G, 19, -3, -7, True, 1), c.want_eval(19, 0, 0, True, 1), "n_iter < 0, top_n < 0")


def test_top_n_on_and_one_past_a_hit(big):
    """top_n equal to a hit's position drops that hit (positions count from 0), one more keeps it"""
    c = big
    K, T, shift = 19, 10, 0
    k = 5                                                           # family 5: the held-out likes
    ids = c.ranked(k, T, True)[0]
    pos = np.flatnonzero(np.isin(ids, c.test_set(k, T, True, shift)))
    assert len(pos) >= 5
    p = int(pos[3])
    below = c.call_eval(c.G, K, T, p, True, shift)
    at = c.call_eval(c.G, K, T, p + 1, True, shift)
    _check(below, c.want_eval(K, T, p, True, shift), ("top_n = position", p))
    _check(at, c.want_eval(K, T, p + 1, True, shift), ("top_n = position + 1", p))
    assert below[0][k] == 3 and at[0][k] == 4 and below[2][k] == p and at[2][k] == p + 1


def test_unnamed_link_types_are_not_excluded(amd):
    """tests/test_gpu_restart_rank.py's case through the evaluating end: every vector's test set is the five targets of u's
    links of types LIKE, 2, 7, 8 and 255; where u is in the set four of them are hits, at the positions of the host's list"""
    c = OddTypes(amd)
    try:
        tests = [c.g["node_id"][c.targets]] * 3
        for top_n in (0, 10):
            got = amd.Recommender(c.H).RecommendationRestartEvalBatch(c.restarts, c.starts, D, c.T, tests, topN=top_n, exclude=c.sets)
            _check(got, [_want(c.lists[k][0], tests[k], top_n) for k in range(3)], ("odd types", top_n))
            if top_n == 0:                                          # the whole lists: the LIKE target alone is missing
                assert got[0].tolist() == [4, 5, 4]
                assert got[2].tolist() == [c.n_items - 1, c.n_items, len(c.lists[2][0])]
    finally:
        c.close()


def test_weighted_graph(amd):
    g = gg.random_graph(33, n_users=250, n_items=700, n_likes=3500, n_etc=8, n_friend=300, n_mention=900, n_author=80)
    assert len(np.unique(g["w"])) > 10
    c = EvalCase(amd, g, 250, 7)
    try:
        c.sweep_eval(16, Ks=(19,), Ts=(1, 10), tops=(0, 100))
        c.sweep_eval(0, Ks=(70,), Ts=(10,), tops=(0,))
    finally:
        c.close()


def test_dangling_users_in_supports_and_sets(amd):
    g = gg.random_graph(34, n_users=400, n_items=600, n_likes=1500, n_friend=40)
    deg = np.diff(g["rowptr"])
    dang = np.flatnonzero(deg[:400] == 0).astype(np.int32)
    assert len(dang) >= 4
    c = EvalCase(amd, g, 400, 8)
    try:
        c.restarts[0] = (np.array([dang[0], 3, dang[1]], dtype=np.int32), np.array([0.5, 0.25, 0.25]))
        c.restarts[1] = (np.array([dang[2]], dtype=np.int32), np.array([1.0]))
        c.starts[1] = dang[2]
        c.starts[2] = dang[3]
        c.sets[1] = np.array([dang[0], dang[1]], dtype=np.int32)
        c.sets[2] = np.array([dang[0], 0], dtype=np.int32)
        c.sweep_eval(4, Ks=(19,), Ts=(0, 1, 10), tops=(0, 100))
    finally:
        c.close()


def test_hub_user_spans_two_segments(amd):
    g0 = gg.random_graph(35, n_users=120, n_items=5200, n_likes=4000, n_friend=60)
    g = _with_hub(g0, 120, 7, 4300)
    assert 4096 < int(g["rowptr"][8] - g["rowptr"][7]) <= 8192
    c = EvalCase(amd, g, 120, 9)
    try:
        c.restarts[0] = (np.array([7, 11], dtype=np.int32), np.array([0.5, 0.5]))
        c.sets[1] = np.array([30, 7, 31], dtype=np.int32)
        c.sets[2] = np.array([7, 7], dtype=np.int32)
        H = amd.Graph.from_flat(**g, tile_seeds=4, tile_group=1)
        H.buildGraph()
        # shift 6 / 5: vector 0 (the hub in its support) and vector 1 (the hub in its set) take the every-item set
        for T, top_n, explicit, shift in ((10, 0, False, 6), (10, 100, True, 5), (1, 0, True, 1), (0, c.n_items + 5, True, 2)):
            _check(c.call_eval(H, 19, T, top_n, explicit, shift), c.want_eval(19, T, top_n, explicit, shift), ("hub", T, top_n, explicit))
        H.close()
    finally:
        c.close()


def test_two_items_share_an_id(amd):
    """a dozen nodes, ITEM nodes 5 and 8 both carry id 77, which is in the test set: both hit, at consecutive positions"""
    U, I = gg.NODE_USER, gg.NODE_ITEM
    node_type = np.array([U, U, U, U, I, I, I, I, I, I, I, I], dtype=np.uint8)
    node_id = np.array([1, 2, 3, 4, 90, 77, 60, 50, 77, 30, 20, 10], dtype=np.int64)
    lists = {0: [4, 6], 1: [6, 7, 9], 2: [9, 10], 3: [11, 4], 4: [0, 3], 5: [], 6: [0, 1], 7: [1], 8: [], 9: [1, 2], 10: [2], 11: [3]}
    g = gg._from_lists(node_id, node_type, lists)
    G = amd.Graph.from_flat(**g)
    G.buildGraph()
    rec = amd.Recommender(G)
    try:
        restarts = [{0: 1.0}, {1: 0.5, 2: 0.5}, {3: 1.0}]
        starts = np.array([-1, -1, 3], dtype=np.int32)
        tests = [[77], [77, 30], [77, 90]]
        for T in (0, 3):
            for K in (3, 1):
                for top_n in (0, 2, 3):
                    want = []
                    for k in range(K):
                        idx, val = list(restarts[k].keys()), list(restarts[k].values())
                        row = _single_row(G, 12, idx, val, int(starts[k]), D, T)
                        ids = _ranked(g, row, np.array(idx))[0]
                        if T == 0 and starts[k] < 0:                # equal scores: the two 77s are neighbours, behind 90
                            assert ids[:3].tolist() == [90, 77, 77] or ids[:2].tolist() == [77, 77]
                        want.append(_want(ids, tests[k], top_n))
                    got = rec.RecommendationRestartEvalBatch(restarts[:K], starts[:K], D, T, tests[:K], topN=top_n)
                    _check(got, want, ("shared id", T, K, top_n))
        # vector 0 at T = 0 excludes items 4 and 6 (ids 90, 60): the list opens with the two 77s
        got = rec.RecommendationRestartEvalBatch(restarts[:2], starts[:2], D, 0, [[77], [77]])
        assert got[0][0] == 2 and got[1][0] == 1.0 / 1 + 2.0 / 2
    finally:
        G.close()


def test_against_the_python_oracle(small):
    """the literal oracle end to end: dense Model.restart, run, exclude over the set, Python sort, evaluate"""
    from tests.test_gpu_restart_batch import _oracle_graph, _oracle_model
    c = small
    PG = _oracle_graph(c.g)
    K, T, shift = 6, 10, 2
    for top_n in (0, 100):
        got = c.call_eval(c.G, K, T, top_n, True, shift)
        for k in range(K):
            idx, val = c.restarts[k]
            m = _oracle_model(PG, D, int(c.starts[k]), idx, val)
            for _ in range(T):
                m.deliverRanks(); m.updateRanks()
            liked = set(_liked(c.g, c.sets[k]).tolist())
            cand = [(float(m.rank[i]), int(c.g["node_id"][i])) for i in range(c.n)
                    if c.g["node_type"][i] == gg.NODE_ITEM and i not in liked]
            cand.sort(key=lambda e: (-e[0], -e[1]))
            if top_n > 0:
                cand = cand[:top_n]
            h, sp = evaluate([(e[1], e[0]) for e in cand], set(int(t) for t in c.test_set(k, T, True, shift)))
            assert (int(got[0][k]), int(got[2][k])) == (h, len(cand)), (k, top_n)
            assert bits(got[1][k:k + 1])[0] == bits(np.array([sp]))[0], (k, top_n)


def test_reduces_to_the_single_seed_evaluation(amd, big):
    """{s: 1.0} with start = s and set {s} at d = (double)(float)0.15, top_n = 0 is rwr_recommend_eval_batch of seed s"""
    c = big
    deg = np.diff(c.g["rowptr"])
    seeds = np.array([s for s in (0, 1, 5, 17, 40, 133, 250, 299, 305, 4000) if deg[s] > 0], dtype=np.int32)
    assert len(seeds) >= 6
    rng = np.random.default_rng(77)
    tests = [rng.choice(c.item_ids, 30, replace=False) for _ in seeds]
    tests[1] = np.zeros(0, dtype=np.int64)
    tests[2] = c.item_ids.copy()
    d = float(np.float32(0.15))
    rec = amd.Recommender(c.G)
    for T in (10, 3):
        want = rec.RecommendationEvalBatch(seeds, 0.15, T, tests)
        assert want[0].sum() > 0
        for exclude in ([[int(s)] for s in seeds], None):
            got = rec.RecommendationRestartEvalBatch([{int(s): 1.0} for s in seeds], seeds, d, T, tests, topN=0, exclude=exclude)
            assert (got[0] == want[0]).all() and (got[2] == want[2]).all(), (T, got, want)
            assert (bits(got[1]) == bits(want[1])).all(), (T, got[1], want[1])


def test_fallbacks_evaluate_the_single_calls_rows(amd, big):
    """K = 1, and a vector of 257 entries (the tolerance class) inside a batch: vector by vector through rwr_model_run_restart"""
    c = big
    rng = np.random.default_rng(23)
    wide = (rng.choice(c.n, 257, replace=False).astype(np.int32), rng.random(257) + 1e-3)
    assert len(wide[0]) == EXACT_MAX + 1
    rs = [c.restarts[3], wide, c.restarts[4], c.restarts[1]]
    st = np.array([-1, 2, 9, -1], dtype=np.int32)
    sets = [c.sets[1], wide[0][:5], np.zeros(0, dtype=np.int32), c.sets[2]]
    tests = [rng.choice(c.item_ids, 40, replace=False), c.item_ids.copy(), np.zeros(0, dtype=np.int64),
             rng.choice(c.item_ids, 40, replace=False)]
    rec = amd.Recommender(c.G)
    T = 4
    rows = [_single_row(c.G, c.n, i, v, int(s), D, T) for (i, v), s in zip(rs, st)]
    for top_n in (0, 100):
        for explicit in (True, False):
            members = sets if explicit else [i for i, _ in rs]
            want = [_want(_ranked(c.g, r, m)[0], t, top_n) for r, m, t in zip(rows, members, tests)]
            got = rec.RecommendationRestartEvalBatch(rs, st, D, T, tests, topN=top_n, exclude=sets if explicit else None)
            _check(got, want, ("wide", top_n, explicit))
        for k in (0, 1):                                            # one vector
            want = [_want(_ranked(c.g, rows[k], sets[k])[0], tests[k], top_n)]
            got = rec.RecommendationRestartEvalBatch([rs[k]], st[k:k + 1], D, T, [tests[k]], topN=top_n, exclude=[sets[k]])
            _check(got, want, ("K=1", k, top_n))


def test_handle_reuse_in_both_directions(amd, small):
    c = small
    g = c.g
    seeds = np.random.default_rng(4).integers(0, c.n, 40).astype(np.int32)

    def evaluated(H):
        return c.call_eval(H, 19, 5, 0, True, 0)

    def ranked(H):
        return c.call(H, 19, 5, 100, True)

    def single_seeds(H):
        return amd.Recommender(H).RecommendationBatch(seeds, 0.15, 10, 20)

    def fresh(f):
        H = amd.Graph.from_flat(**g, tile_seeds=16)
        H.buildGraph()
        try:
            return f(H)
        finally:
            H.close()

    want = {f: fresh(f) for f in (evaluated, ranked, single_seeds)}
    _check(want[evaluated], c.want_eval(19, 5, 0, True, 0), "fresh handle")
    for first, second in ((evaluated, ranked), (evaluated, single_seeds), (ranked, evaluated), (single_seeds, evaluated),
                          (evaluated, evaluated)):
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
    ts = [[1007], [], [1014, 1021]]

    def still_right():
        _check(c.call_eval(G, 19, 1, 0, True, 0), c.want_eval(19, 1, 0, True, 0), "after a refused call")

    def refused(status, *words, restarts=ok, starts=None, d=D, T=3, tests=ts, exclude=None):
        with pytest.raises(amd.RwrError) as ei:
            rec.RecommendationRestartEvalBatch(restarts, starts, d, T, tests[:len(restarts)], exclude=exclude)
        assert ei.value.status == status, str(ei.value)
        for w in ("rwr_recommend_restart_eval_batch",) + words:
            assert w in str(ei.value), (w, str(ei.value))

    # what rwr_recommend_restart_batch reports for the vectors and the sets, with the same status and the batch position
    refused(_lib.RWR_E_INVALID, "index 4", "vector 1", restarts=[ok[0], ([4, 9, 4], [1.0, 2.0, 3.0]), ok[2]])
    refused(_lib.RWR_E_RANGE, "batch position 2", restarts=[ok[0], ok[1], ([4, n], [1.0, 2.0])])
    refused(_lib.RWR_E_RANGE, "batch position 1", starts=[0, n, -1])
    for bad in (np.inf, np.nan):
        refused(_lib.RWR_E_UNSUPPORTED, "restart", "batch position 1", restarts=[ok[0], ([4, 9], [0.5, bad])])
    refused(_lib.RWR_E_UNSUPPORTED, "negative", "batch position 2", restarts=[ok[0], ok[1], ([4, 9], [0.5, -1e-300])])
    for d in (-0.01, 1.5, np.nan):
        refused(_lib.RWR_E_UNSUPPORTED, "damping factor", d=d)
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
        amd.Recommender(H).RecommendationRestartEvalBatch(ok, None, D, 3, ts)
    assert ei.value.status == _lib.RWR_E_UNSUPPORTED and "non-negative" in str(ei.value)
    H.close()

    # the raw entry: pointers, K, the test sets, and that a refused call writes nothing
    lib = _lib.load()
    ptr, idx, val = np.array([0, 1, 2], dtype=np.int64), np.array([1, 2], dtype=np.int32), np.array([1.0, 1.0])
    hits, sp, ln = np.full(2, 7, dtype=np.int64), np.full(2, 7.0), np.full(2, 7, dtype=np.int64)
    tp, ti = np.array([0, 1, 2], dtype=np.int64), np.array([1007, 1014], dtype=np.int64)
    pp, pi, pv = ptr.ctypes.data_as(PI64), idx.ctypes.data_as(PI32), val.ctypes.data_as(PD)
    ph, ps, pl = hits.ctypes.data_as(PI64), sp.ctypes.data_as(PD), ln.ctypes.data_as(PI64)
    ptp, pti = tp.ctypes.data_as(PI64), ti.ctypes.data_as(PI64)
    h, call = G._handle(), lib.rwr_recommend_restart_eval_batch
    assert call(h, -1, pp, pi, pv, None, None, None, D, 3, 0, ptp, pti, ph, ps, pl) == _lib.RWR_E_INVALID
    assert b"negative K" in lib.rwr_last_error()
    assert call(h, 0, None, None, None, None, None, None, D, 3, 0, None, None, None, None, None) == _lib.RWR_OK
    assert call(h, 2, None, pi, pv, None, None, None, D, 3, 0, ptp, pti, ph, ps, pl) == _lib.RWR_E_INVALID
    assert call(h, 2, pp, None, pv, None, None, None, D, 3, 0, ptp, pti, ph, ps, pl) == _lib.RWR_E_INVALID
    for args, word in (((None, pti, ph, ps, pl), b"test_ptr"), ((ptp, pti, None, ps, pl), b"n_hits"),
                       ((ptp, pti, ph, None, pl), b"sum_precision"), ((ptp, None, ph, ps, pl), b"test_ids")):
        assert call(h, 2, pp, pi, pv, None, None, None, D, 3, 0, *args) == _lib.RWR_E_INVALID
        assert b"rwr_recommend_restart_eval_batch" in lib.rwr_last_error() and word in lib.rwr_last_error()
    for bad_ptr in ([1, 1, 2], [0, 2, 1]):
        bp = np.array(bad_ptr, dtype=np.int64)
        assert call(h, 2, pp, pi, pv, None, None, None, D, 3, 0, bp.ctypes.data_as(PI64), pti, ph, ps, pl) == _lib.RWR_E_INVALID
        assert b"test_ptr" in lib.rwr_last_error()
        assert call(h, 2, pp, pi, pv, None, bp.ctypes.data_as(PI64), pi, D, 3, 0, ptp, pti, ph, ps, pl) == _lib.RWR_E_INVALID
        assert b"excl_ptr" in lib.rwr_last_error()
    big_ptr = np.array([0, 2 ** 31, 2 ** 31 + 1], dtype=np.int64)      # (the ids of such a set are never read)
    assert call(h, 2, pp, pi, pv, None, None, None, D, 3, 0, big_ptr.ctypes.data_as(PI64), pti, ph, ps, pl) == _lib.RWR_E_UNSUPPORTED
    assert b"INT32_MAX" in lib.rwr_last_error()
    assert (hits == 7).all() and (sp == 7.0).all() and (ln == 7).all(), "a refused call wrote results"
    # empty test sets with a NULL id array, a NULL list_len
    zp = np.zeros(3, dtype=np.int64)
    assert call(h, 2, pp, pi, pv, None, None, None, D, 3, 0, zp.ctypes.data_as(PI64), None, ph, ps, None) == _lib.RWR_OK
    assert (hits == 0).all() and (sp == 0.0).all() and (ln == 7).all()
    assert call(h, 2, pp, pi, pv, None, None, None, D, 3, 0, zp.ctypes.data_as(PI64), None, ph, ps, pl) == _lib.RWR_OK
    assert (ln > 0).all()
    # K = 0 through the mirror
    e = rec.RecommendationRestartEvalBatch([], None, D, 3, [])
    assert e[0].shape == (0,) and e[1].shape == (0,) and e[2].shape == (0,)
    still_right()
