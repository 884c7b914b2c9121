"""Crafted rank vectors for ONE Model.deliverRanks step of the single-seed seed-row chain (chain_scan.hip: k_cs_block1 /
k_cs_carry1), one case per branch of its decision tree, with a plain sequential reference.  Pure Python / numpy: no GPU
import.  tests/test_chain_cases.py proves every case's claims on the CPU, tests/test_gpu_chain_edges.py runs the cases.

How a case steers the chain (d = 0.5, every weight 1, every row's link count a power of two, so all of this is exact):
  * a row without links is dangling and adds exactly rank[i] to the seed's row (Model.cs:96-97);
  * a row with links holds rank[i] = 2a and adds  2a - fl(0.5 * 2a) = a  (Model.cs:91-93);
  * each of its links into the seed adds  fl(fl(0.5 * 2a) * (1 / links)) = a / links,  in front of the row's own addend
    (Model.cs:85-88).
Within four rows of a block edge a row is linked when row % 3 == 1 and dangling otherwise (so both kinds stand on both sides
of every edge); elsewhere only the rows with a link into the seed are linked.  One row away from every edge under test
(`wrow`) has one link; the weighted form of a case gives it a second link of another weight, which takes the whole graph off the value-free kernels
and leaves the seed row's addends as they were.

predict() is an executable model of the kernels' decisions (which kind k_cs_block1 gives each block, what k_cs_carry1 does
with it) for a given way of forming the APPROXIMATE block sums -- the kernels may associate those in any order, so a claim
about a kind or a redo count only stands when predict() gives it for every method in APPROX."""
import math

import numpy as np

from tests import binade_scan_model as bsm

# the constants of chain_scan.hip the cases are built around (tests/test_chain_cases.py reads them out of the source)
EXPECTED_CONSTANTS = {"BLOCK_ROWS": 1024, "FEW": 64, "CS_MX_LINKS": 8192, "CS_RUN_ADDENDS": 8, "own_max": 48, "WINDOW": 64}
B = EXPECTED_CONSTANTS["BLOCK_ROWS"]
FEW = EXPECTED_CONSTANTS["FEW"]
MX = EXPECTED_CONSTANTS["CS_MX_LINKS"]
RUN = EXPECTED_CONSTANTS["CS_RUN_ADDENDS"]
OWN = EXPECTED_CONSTANTS["own_max"]
W = EXPECTED_CONSTANTS["WINDOW"]
D = 0.5

NODE_USER, NODE_ITEM = 1, 2
BIG = bsm.BIG


def _exp(x):
    return (bsm.bits(x) >> 52) & 0x7FF


def _mant(x):
    return (bsm.bits(x) & ((1 << 52) - 1)) | (1 << 52)


def _from_m(eb, M):
    return bsm.from_bits((eb << 52) | (M - (1 << 52)))


def fold(seq, s=0.0):
    for a in seq:
        s = s + a
    return s


# ------------------------------------------------------------------------------------------------------ building a case

class Case:
    """name, n, seed, d, x (the rank vector), lists (row -> [(target, type, weight)]), claims; flat(weighted) = the graph."""

    def __init__(self, name, n, seed, x, lists, wrow, claims):
        self.name, self.n, self.seed, self.d, self.x, self.lists, self.wrow, self.claims = name, n, seed, D, x, lists, wrow, claims
        self._flat = {}

    def flat(self, weighted=False):
        if weighted not in self._flat:
            n = self.n
            rowptr = np.zeros(n + 1, dtype=np.int64)
            dst, et, w = [], [], []
            rows = sorted(self.lists)
            cnt = np.zeros(n, dtype=np.int64)
            for i in rows:
                ls = list(self.lists[i])
                if weighted and i == self.wrow:
                    ls.append((self.claims["sink2"], 2, 3.0))
                for (t, y, wt) in ls:
                    dst.append(t); et.append(y); w.append(wt)
                cnt[i] = len(ls)
            rowptr[1:] = np.cumsum(cnt)
            node_type = np.full(n, NODE_USER, dtype=np.uint8)
            node_type[n // 2:] = NODE_ITEM
            self._flat[weighted] = dict(node_id=np.arange(n, dtype=np.int64) * 3 + 11, node_type=node_type, rowptr=rowptr,
                                        dst=np.array(dst, dtype=np.int32), etype=np.array(et, dtype=np.uint8),
                                        w=np.array(w, dtype=np.float64))
        return self._flat[weighted]


class Builder:
    """Rows in ascending order; tracks the seed row's sequential sum so that a case can place an addend relative to it."""

    def __init__(self, name, n, seed=5, wrow=300, sink=6, sink2=7):
        assert seed % 3 != 1 and sink != seed and sink2 != seed
        self.name, self.n, self.seed, self.wrow, self.sink, self.sink2 = name, n, seed, wrow, sink, sink2
        self.x = np.zeros(n, dtype=np.float64)
        self.lists = {}
        self.i = 0
        self.s = 0.0

    def _linked_by_pattern(self, i):
        return i == self.wrow or (i % 3 == 1 and i != self.seed and (i % B < 4 or i % B >= B - 4))

    def row(self, a, seed_links=0, links=None):
        """The next row adds `a` to the seed's row behind `seed_links` links into the seed (a / links each; links = a power of
        two >= seed_links, the others go to the sink)."""
        i = self.i
        assert i < self.n
        a = float(a)
        if links is None:
            links = 1
            while links < seed_links:
                links *= 2
        linked = seed_links > 0 or self._linked_by_pattern(i)
        if linked:
            assert i != self.seed and links & (links - 1) == 0 and (i != self.wrow or seed_links == 0)
            self.x[i] = 2.0 * a
            assert self.x[i] - 0.5 * self.x[i] == a and (0.5 * self.x[i]) * (1.0 / links) * links == a
            self.lists[i] = [(self.seed, 1 + q % 7, 1.0) for q in range(seed_links)] + \
                            [(self.sink, 1 + q % 7, 1.0) for q in range(links - seed_links)]
            for _ in range(seed_links):
                self.s = self.s + a / links
        else:
            self.x[i] = a
        self.s = self.s + a
        self.i += 1
        return i

    def rows(self, seq):
        for a in seq:
            self.row(a)

    def zeros_to(self, i):
        """all-zero rows up to (not including) row i: dangling, except the pattern's linked rows next to a block edge"""
        assert self.i <= i <= self.n
        for e in range((self.i // B) * B, i + B, B):
            for j in range(e - 3, e + 4):
                if self.i <= j < i and self._linked_by_pattern(j):
                    self.lists[j] = [(self.sink, 1, 1.0)]
        if self.i <= self.wrow < i:
            self.lists[self.wrow] = [(self.sink, 1, 1.0)]
        self.i = i

    def level(self):
        """One row that brings the sum to exactly 1.5 * 2^E (exactly: Sterbenz); returns ulp = 2^(E - 52)."""
        m, e = math.frexp(self.s)                # s = m * 2^e, 0.5 <= m < 1
        T = math.ldexp(0.75, e) if m <= 0.75 else math.ldexp(1.5, e)
        a = T - self.s
        self.row(a)
        assert self.s == T
        return math.ldexp(1.0, (e - 1 if m <= 0.75 else e) - 52)

    def done(self, **claims):
        self.zeros_to(self.n)
        claims.setdefault("redo", "open")            # "zero": == 0, "some": >= 1, "open": recorded only
        claims.setdefault("order_exempt", None)      # a reason, where the sum cannot depend on the order
        claims["sink2"] = self.sink2
        return Case(self.name, self.n, self.seed, self.x, self.lists, self.wrow, claims)


def noisy(rng, count, lo=-30, hi=30):
    """magnitudes over 60 binades with a few mantissa bits: sums that round at nearly every add"""
    return np.ldexp(1.0 + rng.integers(0, 8, count) / 8.0, rng.integers(lo, hi, count).astype(np.int32)).tolist()


def filler(rng, count, u):
    """addends around one ulp of the running sum: exact halves (ties, both parities), near-halves, small multiples"""
    return (rng.choice([0.0, 0.5, 0.5, 0.75, 1.25, 1.5, 2.5, 3.0], size=count) * u).tolist()


# ---------------------------------------------------------------------------------------------------------- the reference

def normalised(flat):
    """Graph.buildGraph (Graph.cs:51-88) on the flat arrays: (w_norm per link, dangling per row)."""
    rowptr, et, w = flat["rowptr"], flat["etype"], flat["w"]
    n = len(rowptr) - 1
    wn = np.zeros(len(w), dtype=np.float64)
    dang = np.ones(n, dtype=bool)
    for i in np.nonzero(np.diff(rowptr))[0].tolist():
        p0, p1 = int(rowptr[i]), int(rowptr[i + 1])
        expl = [p for p in range(p0, p1) if et[p] != 0]
        if expl:
            sw = 0.0
            for p in expl:
                sw += float(w[p])                     # Graph.cs:70-77
            for p in expl:
                wn[p] = float(w[p]) / sw              # Graph.cs:80-81
            dang[i] = False
    return wn, dang


def seed_row_rows(case, weighted=False):
    """Per row, the addends it gives the seed's row in the reference's order: its links into the seed in list order
    (Model.cs:85-88), then its restart addend (Model.cs:91-93 / 96-97)."""
    flat = case.flat(weighted)
    wn, dang = normalised(flat)
    rowptr, dst, et = flat["rowptr"], flat["dst"], flat["etype"]
    c1 = 1 - case.d
    out = []
    for i in range(case.n):
        xi = float(case.x[i])
        if dang[i]:
            out.append([xi])
            continue
        rw = c1 * xi                                  # Model.cs:84
        r = [rw * float(wn[p]) for p in range(int(rowptr[i]), int(rowptr[i + 1])) if et[p] != 0 and dst[p] == case.seed]
        r.append(xi - rw)                             # Model.cs:91
        out.append(r)
    return out


def seed_row_addends(case, weighted=False):
    return [a for r in seed_row_rows(case, weighted) for a in r]


def deliver_reference(case, weighted=False):
    """The whole nextRank of one deliverRanks on rank = x: the seed's row is the left fold of seed_row_addends, every other
    row the list-order sum of its in-links' fl(fl((1 - d) * x[src]) * w)."""
    flat = case.flat(weighted)
    wn, dang = normalised(flat)
    rowptr, dst = flat["rowptr"], flat["dst"]
    c1 = 1 - case.d
    out = [0.0] * case.n
    for i in np.nonzero(~dang)[0].tolist():
        rw = c1 * float(case.x[i])
        for p in range(int(rowptr[i]), int(rowptr[i + 1])):
            t = int(dst[p])
            if t != case.seed and wn[p] != 0.0:
                out[t] = out[t] + rw * float(wn[p])
    out[case.seed] = fold(seed_row_addends(case, weighted))
    return np.array(out, dtype=np.float64)


# --------------------------------------------------------------------------- what the kernels decide (executable model)

def _sum_fsum(v):
    return math.fsum(v)


def _sum_pairwise(v):
    return float(np.sum(np.array(v, dtype=np.float64))) if len(v) else 0.0


def _sum_reversed(v):
    return fold(reversed(list(v)))


APPROX = {"fsum": _sum_fsum, "pairwise": _sum_pairwise, "reversed": _sum_reversed}


def _pf(rows, eb):
    f = (0, 0)
    for r in rows:
        for a in r:
            if a != 0.0:
                f = bsm.compose(f, bsm.addend_func(a, eb))
    return f


def _locate(rows, start, mt, eb):
    """k_cs_block1's locate(): the first row at which the approximate mantissa mt leaves binade eb -> (row, function of the
    rows in front of it from `start` on)"""
    running = (0, 0)
    for r in range(start, len(rows)):
        incu = bsm.compose(running, _pf([rows[r]], eb))
        if mt + running[0] < BIG <= mt + incu[0]:
            return r, running
        running = incu
    return None


def block_pass(rows, pre, ap):
    """k_cs_block1 for one block: its rows' addend lists, the approximate sum in front of it and its own."""
    if ap == 0.0:
        return {"kind": "ZERO"}
    if pre == 0.0:
        return {"kind": "EXACT", "ex": fold(a for r in rows for a in r)}
    epre, epost = _exp(pre), _exp(pre + ap)
    if epre == 0 or epost >= 0x7FF or epost > epre + 2:
        return {"kind": "REDO", "eb": epre}
    plain = {"kind": "PLAIN", "eb": epre, "f": _pf(rows, epre)}
    if epost == epre:
        return plain
    mt = _mant(pre)
    loc = _locate(rows, 0, mt, epre)
    if loc is None:
        return dict(plain, unlocated=True)
    r1, before = loc
    if len(rows[r1]) > RUN:
        return {"kind": "REDO", "eb": epre}
    split = {"kind": "SPLIT", "eb": epre, "before": before, "rows": rows[r1], "after": _pf(rows[r1 + 1:], epre + 1), "row": r1}
    if epost == epre + 1:
        return split
    s1 = fold(rows[r1], _from_m(epre, mt + before[0]))
    if _exp(s1) != epre + 1 or epre + 2 >= 0x7FF:
        return {"kind": "REDO", "eb": epre}
    loc2 = _locate(rows, r1 + 1, _mant(s1), epre + 1)
    if loc2 is None:
        return split
    r2, middle = loc2
    if len(rows[r2]) > RUN:
        return {"kind": "REDO", "eb": epre}
    return {"kind": "SPLIT2", "eb": epre, "before": before, "rows1": rows[r1], "middle": middle, "rows2": rows[r2],
            "after": _pf(rows[r2 + 1:], epre + 2), "row": r1, "row2": r2}


def predict(rows, approx="fsum"):
    """The single-seed chain on the per-row addend lists: {"sum", "redo" (what chain_redo_blocks counts), "kinds" (per block),
    "redone" (blocks the carry redid), "cells"}.  One block: the direct walk, which counts no redo."""
    sumf = APPROX[approx]
    n = len(rows)
    nb = -(-n // B)
    if nb == 1:
        return {"sum": fold(a for r in rows for a in r), "redo": 0, "kinds": ["DIRECT"], "redone": [], "cells": [None]}
    blocks = [rows[c * B:(c + 1) * B] for c in range(nb)]
    aps = [sumf([a for r in blk for a in r]) for blk in blocks]
    cells = [block_pass(blocks[c], sumf(aps[:c]), aps[c]) for c in range(nb)]
    s, redone = 0.0, []
    for c, cell in enumerate(cells):
        kind = cell["kind"]
        if kind == "ZERO":
            continue
        eb = _exp(s)
        normal = eb != 0 and eb != 0x7FF
        t = None
        if kind == "PLAIN" and normal and cell["eb"] == eb:
            t = bsm.apply_block(s, [cell["f"]])
        elif kind == "EXACT" and bsm.bits(s) == 0:
            t = cell["ex"]
        elif kind == "SPLIT" and normal and eb + 2 < 0x7FF:
            t = bsm.apply_split(s, cell)
        elif kind == "SPLIT2" and normal and eb + 2 < 0x7FF:
            t = bsm.apply_split2(s, cell)
        if t is None:
            t = fold((a for r in blocks[c] for a in r), s)       # cs_redo_block: exact by construction
            redone.append(c)
        s = t
    return {"sum": s, "redo": len(redone), "kinds": [c["kind"] for c in cells], "redone": redone, "cells": cells}


# --------------------------------------------------------------------------------------------------------------- the cases

def _head(b, rng, count=40):
    """order-sensitive addends, then one that levels the sum to 1.5 * 2^E; returns that binade's ulp"""
    b.rows(noisy(rng, count))
    return b.level()


def _geometry(name, n, rng, events):
    """head in block 0, ulp-sized addends in every other row, and at the rows of `events`: "cross", one addend of half the sum
    (a clean crossing), or "jump", one of 16 times the sum (the block's predicted exponents differ by more than 2: CS_REDO)"""
    b = Builder(name, n)
    u = _head(b, rng)
    for at in sorted(events):
        b.rows(filler(rng, at - b.i, u))
        if events[at] == "cross":
            b.row(b.s * 0.5)
            u *= 2
        else:
            b.row(16.0 * b.s)
            u *= 16
    b.rows(filler(rng, n - b.i, u))
    return b


def make_cases():
    rng = np.random.default_rng(20240607)
    cases = []

    # ---- launch form and geometry
    for n in (B - 1, B):                                  # one block: the direct walk (the carry alone; no redo is counted)
        b = Builder(f"direct_n{n}", n)
        b.rows(noisy(rng, n))
        cases.append(b.done(redo="zero", kinds={0: "DIRECT"}, branch="direct walk (one block)"))
    b = Builder(f"two_blocks_n{B + 1}", B + 1)            # two blocks, the last of a single row
    b.rows(noisy(rng, B))
    b.row(1.375 * 2.0 ** 28)
    cases.append(b.done(redo="zero", kinds={0: "EXACT", 1: "PLAIN"}, branch="exact start + a last block of one row (own sums)"))
    for n, what in ((OWN * B, "own sums, 48 blocks"), (OWN * B + 1, "separate approximate pass, 49 blocks")):
        b = _geometry(f"blocks_n{n}", n, rng, {40 * B + 517: "cross"})
        cases.append(b.done(redo="zero", kinds={0: "EXACT", 1: "PLAIN", 40: "SPLIT", OWN - 1: "PLAIN"}, crossings=[(40, 517)], branch=what))
    for n, what in ((W * B, "one carry window exactly"), (W * B + 1, "a second window of one block of one row")):
        b = _geometry(f"window_n{n}", n, rng, {(W - 2) * B + 517: "cross"})
        cases.append(b.done(redo="zero", kinds={0: "EXACT", W - 2: "SPLIT", W - 1: "PLAIN"}, crossings=[(W - 2, 517)], branch=what))
    b = _geometry("redo_last_of_window", W * B + 1, rng, {(W - 1) * B: "jump"})
    cases.append(b.done(redo="some", redone=[W - 1], kinds={W - 1: "REDO", W: "PLAIN"}, branch="CS_REDO block is the last of the first window"))
    b = _geometry("redo_first_of_next_window", W * B + 1, rng, {W * B: "jump"})
    cases.append(b.done(redo="some", redone=[W], kinds={W - 1: "PLAIN", W: "REDO"}, branch="CS_REDO block (one row) is the first of the second window"))

    # ---- exact-start block
    b = Builder("all_zero_ranks", 2 * B + 77)
    cases.append(b.done(redo="zero", kinds={0: "ZERO", 1: "ZERO", 2: "ZERO"}, zero_blocks=[0, 1, 2], order_exempt="every addend is +0.0",
                        branch="every block a no-op (CS_PLAIN with a zero sum)"))
    b = Builder("exact_start_block3", 4 * B + 37)
    b.zeros_to(3 * B)
    u = _head(b, rng, 700)
    b.rows(filler(rng, b.n - b.i, u))
    cases.append(b.done(redo="zero", kinds={0: "ZERO", 1: "ZERO", 2: "ZERO", 3: "EXACT", 4: "PLAIN"}, zero_blocks=[0, 1, 2],
                        links_per_block={3: 0}, branch="leading all-zero blocks, exact start in block 3, no link into the seed"))
    b = Builder("exact_start_last_block", 2 * B + 500)
    b.zeros_to(2 * B + 3)
    b.rows(noisy(rng, 480))
    cases.append(b.done(redo="zero", kinds={0: "ZERO", 1: "ZERO", 2: "EXACT"}, zero_blocks=[0, 1], branch="exact start in the last block"))
    b = Builder("zero_blocks_in_the_middle", 4 * B + 11)
    u = _head(b, rng, 900)
    b.zeros_to(3 * B + 2)
    b.rows(filler(rng, b.n - b.i, u))
    cases.append(b.done(redo="zero", kinds={0: "EXACT", 1: "ZERO", 2: "ZERO", 3: "PLAIN", 4: "PLAIN"}, zero_blocks=[1, 2],
                        branch="all-zero blocks behind the exact start"))
    for nl in (FEW, FEW + 1, MX, MX + 1):
        # the seed sits in block 1, every link into it comes from block 0; sources on the block's first and last row
        b = Builder(f"exact_start_{nl}_links", 2 * B + 77, seed=B + 5, wrow=B + 300, sink=B + 6, sink2=B + 7)
        per = [0] * B
        if nl <= B:
            for r in [0, B - 1] + list(range(7, 7 + 16 * (FEW - 2), 16)):
                per[r] = 1
            if nl == FEW + 1:
                per[0] = 2                                 # several links from one source row
        else:
            for r in [0] + list(range(3, B, 2)):           # 16 each from half the rows (the types repeat: the flat arrays
                per[r] = 2 * MX // B                       # take multi-edges, and so does the oracle)
            if nl == MX + 1:
                per[17] += 1
        assert sum(per) == nl
        for r, a in enumerate(noisy(rng, B, -20, 20)):
            b.row(a, seed_links=per[r])
        u = b.level()
        b.rows(filler(rng, b.n - b.i, u))
        form = "FEW table in LDS" if nl <= FEW else "staged in the scratch row" if nl <= MX else "walked through global memory"
        cases.append(b.done(redo="zero", kinds={0: "EXACT"}, links_per_block={0: nl, 1: 0, 2: 0},
                            branch=f"exact start with {nl} links into the seed: {form}"))
    b = Builder("only_inlink_from_last_row", 2 * B + 77)
    u = _head(b, rng, 800)
    b.rows(filler(rng, b.n - 1 - b.i, u))
    b.row(5.5 * u, seed_links=1)
    cases.append(b.done(redo="zero", kinds={0: "EXACT", 1: "PLAIN", 2: "PLAIN"}, links_per_block={0: 0, 1: 0, 2: 1},
                        branch="the seed's only in-link comes from row n - 1 (a plain block's run function)"))

    # ---- predicted crossings that hold
    for name, at in (("cross_in_first_run", B + 1), ("cross_in_last_run", 2 * B - 3), ("cross_in_last_row", 2 * B - 1),
                     ("cross_in_first_row_of_next_block", 2 * B)):
        b = Builder(name, 3 * B + 101)
        u = _head(b, rng, 600)
        b.rows(filler(rng, at - b.i, u))
        b.row(b.s * 0.5)
        b.rows(filler(rng, b.n - b.i, 2 * u))
        c = at // B
        cases.append(b.done(redo="zero", kinds={0: "EXACT", c: "SPLIT", 3 - c: "PLAIN", 3: "PLAIN"}, crossings=[(c, at % B)],
                            branch=f"one predicted crossing at row {at % B} of block {c}"))
    # the sum reaches exactly 2^(E+1) on block 1's last addend.  Blocks 0 and 1 hold multiples of one quantum only, so that
    # every association of the approximate sums is exact and the prediction does not hang on a rounding
    b = Builder("power_of_two_on_last_addend", 3 * B + 101)
    b.rows((rng.integers(1, 9, B - 1) * 2.0 ** -20).tolist())
    u = b.level()
    b.rows((rng.integers(0, 9, B - 1) * (2.0 ** 20 * u)).tolist())
    e2 = math.ldexp(1.0, math.frexp(b.s)[1])
    b.row(e2 - b.s)
    assert b.s == e2 and b.i == 2 * B
    b.rows(filler(rng, b.n - b.i, 2 * u))
    cases.append(b.done(redo="zero", kinds={0: "EXACT", 1: "SPLIT", 2: "PLAIN"}, crossings=[(1, B - 1)], power_of_two_after=2 * B - 1,
                        branch="m' = 2^53 exactly on a block's last addend"))
    # exact half-ulp addends on either parity of the running mantissa, directly before and directly behind a block edge (a tie
    # always leaves an even mantissa, so an odd one needs the row in front of it)
    for name, ctl, odd, ties in (("half_ulp_before_edge_odd", 2 * B - 2, 1, [(2 * B - 1, 1), (2 * B, 0)]),
                                 ("half_ulp_before_edge_even", 2 * B - 2, 0, [(2 * B - 1, 0), (2 * B, 0)]),
                                 ("half_ulp_behind_edge_odd", 2 * B - 1, 1, [(2 * B, 1), (2 * B + 1, 0)])):
        b = Builder(name, 3 * B + 101)
        u = _head(b, rng, 600)
        b.rows(filler(rng, ctl - b.i, u))
        b.row((2 - (_mant(b.s) & 1) + odd) * u)            # leaves a mantissa of the wanted parity
        b.rows([0.5 * u, 0.5 * u])
        b.rows(filler(rng, b.n - b.i, u))
        cases.append(b.done(redo="zero", kinds={0: "EXACT", 1: "PLAIN", 2: "PLAIN", 3: "PLAIN"}, ties=ties,
                            branch="half-ulp addends at a block edge (plain blocks): " + name))
    # ... and inside the crossing row: a link into the seed whose addend is a tie in the old binade, then the row's own addend,
    # which crosses -- from an even and from an odd mantissa
    for name, odd in (("link_and_half_ulp_in_the_crossing_row_even", 0), ("link_and_half_ulp_in_the_crossing_row_odd", 1)):
        b = Builder(name, 3 * B + 101)
        u = _head(b, rng, 600)
        b.rows(filler(rng, B + 400 - b.i, u))
        b.row((2 - (_mant(b.s) & 1) + odd) * u)
        a = b.s / 4.0                                      # link addend a, then restart addend a
        a = _from_m(_exp(a), _mant(a) & ~((1 << 22) - 1)) + 0.5 * u      # a = (a multiple of 2^20 ulps) + half an ulp
        at = b.row(a, seed_links=1)
        b.rows(filler(rng, b.n - b.i, 2 * u))
        cases.append(b.done(redo="zero", kinds={0: "EXACT", 1: "SPLIT", 2: "PLAIN"}, crossings=[(1, at % B)], ties=[(at, odd)],
                            links_per_block={1: 1},
                            branch="a link into the seed and a half-ulp tie inside the crossing row (CS_SPLIT hands over the row's addends)"))
    b = Builder("two_crossings_in_one_block", 3 * B + 101)
    u = _head(b, rng, 600)
    b.rows(filler(rng, B + 100 - b.i, u))
    b.row(b.s * 0.5)
    b.rows(filler(rng, B + 600 - b.i, 2 * u))
    b.row(b.s)
    b.rows(filler(rng, b.n - b.i, 4 * u))
    cases.append(b.done(redo="zero", kinds={0: "EXACT", 1: "SPLIT2", 2: "PLAIN"}, crossings=[(1, 100), (1, 600)],
                        branch="two predicted crossings in one block behind the first (CS_SPLIT2)"))

    # ---- predictions that must fail and be redone
    # (a) the plain block sums keep what the sequential chain drops: eight blocks of quarter-ulps push the predicted crossing
    #     row of block 9 (64 ulps per row) 32 rows in front of the true one
    b = Builder("drift_moves_the_crossing_row", 11 * B + 3)
    b.rows(noisy(rng, 300))
    u = b.level()
    b.rows([0.0] * (B - b.i))
    b.row(b.s / 3.0 - 500 * 64 * u)                        # -> 2^(E+1) - 500 * 64 ulps
    b.rows([0.25 * u] * (9 * B - b.i))
    b.rows([64.0 * u] * B)
    b.rows(filler(rng, b.n - b.i, 2 * u))
    cases.append(b.done(redo="some", redone=[9], kinds={0: "EXACT", 8: "PLAIN", 9: "SPLIT", 10: "PLAIN"}, crossings=[(9, 499)],
                        mispredicted_row=(9, 8), branch="CS_SPLIT on a row >= 8 rows from the true crossing: the carry's check fails"))
    # (b) predicted to cross, does not: 2 - 2^-52 followed by 2^-54 s
    b = Builder("predicted_crossing_that_never_comes", 3 * B + 101)
    b.rows([2.0 ** -k for k in range(53)])
    assert b.s == 2.0 - 2.0 ** -52
    b.rows([0.0] * (B - b.i))
    b.rows([2.0 ** -54] * (b.n - b.i))
    cases.append(b.done(redo="some", redone=[2, 3], kinds={0: "EXACT", 1: "PLAIN", 2: "PLAIN", 3: "PLAIN"}, crossings=[], unlocated=[1],
                        branch="the approximate sums leave the binade, the scan does not (block 1); blocks 2, 3 carry the wrong binade"))
    # (c) predicted plain, crosses: 0.75-ulp addends count one ulp each in the chain and 0.75 in the block sums
    b = Builder("unpredicted_crossing", 3 * B + 101)
    b.rows(noisy(rng, 300))
    u = b.level()
    b.rows([0.0] * (B - 1 - b.i))
    b.row(b.s / 3.0 - 900 * u)                             # -> 2^(E+1) - 900 ulps
    b.rows([0.75 * u] * B)
    b.rows(filler(rng, b.n - b.i, 2 * u))
    cases.append(b.done(redo="some", redone=[1, 2], kinds={0: "EXACT", 1: "PLAIN", 2: "SPLIT", 3: "PLAIN"}, crossings=[(1, 899)],
                        branch="a block predicted plain crosses: the carry's end check fails; block 2 then carries the wrong binade"))
    b = Builder("nine_addends_in_the_crossing_row", 3 * B + 101)
    u = _head(b, rng, 600)
    b.rows(filler(rng, B + 400 - b.i, u))
    at = b.row(b.s * 0.5, seed_links=RUN)                  # 8 links into the seed + the restart addend
    b.rows(filler(rng, b.n - b.i, 2 * u))
    cases.append(b.done(redo="some", redone=[1], kinds={0: "EXACT", 1: "REDO", 2: "PLAIN"}, links_per_block={1: RUN},
                        branch="the crossing row has more than CS_RUN_ADDENDS addends: CS_REDO"))
    b = Builder("three_crossings_in_one_block", 3 * B + 101)
    u = _head(b, rng, 600)
    b.rows(filler(rng, B + 100 - b.i, u))
    for k in range(3):
        b.row(b.s)
        b.rows(filler(rng, 200, u * 2 ** (k + 1)))
    b.rows(filler(rng, b.n - b.i, 8 * u))
    cases.append(b.done(redo="some", redone=[1], kinds={0: "EXACT", 1: "REDO", 2: "PLAIN"}, crossings=[(1, 100), (1, 301), (1, 502)],
                        branch="more than two crossings in one block: CS_REDO"))
    b = Builder("subnormal_incoming_sum", 2 * B + 77)
    b.rows((rng.integers(0, 9, B) * 5e-324).tolist())
    b.rows(noisy(rng, b.n - b.i))
    cases.append(b.done(redo="some", redone=[1], kinds={0: "EXACT", 1: "REDO"}, branch="a subnormal sum enters block 1: CS_REDO"))
    b = Builder("binade_every_few_rows", 3 * B + 9)
    b.rows(np.ldexp(1.0 + rng.random(b.n), (np.minimum(np.arange(b.n), b.n - 300) // 4 - 400 + rng.integers(0, 3, b.n)).astype(np.int32)).tolist())
    cases.append(b.done(redo="some", redone=[1, 2], kinds={0: "EXACT", 1: "REDO", 2: "REDO"},
                        branch="magnitudes over hundreds of binades, a crossing every few rows (the last 300 rows level off): CS_REDO"))
    return cases


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = make_cases()
    return _CASES
