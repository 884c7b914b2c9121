"""Crafted graphs and rank vectors for ONE Model.deliverRanks step of the single-seed SpMV (spmv.hip: k_spmv_exact_binned,
k_spmv_exact_hub; sweep.hip: the table kernels and k_sweep_lds), one case per decision point of that code, with a plain
sequential reference.  Pure Python / numpy: no GPU import.  tests/test_spmv_cases.py proves every case's claims on the CPU
(there lives the model of the device's layout), tests/test_gpu_spmv_edges.py and tests/spmv_edges_child.py run the cases.

A case is a flat graph given by the IN-lists of its rows (row j <- ascending sources), a seed, a rank vector x >= 0, d, the
knob sets it is meant for and a dict of claims.  The operation is a dense step: nextRank[j] = the list-order sum over the
in-links (u -> j) of fl(fl((1 - d) * x[u]) * w), and the seed's row the seed-row chain's left fold (tests/chain_cases.py).
Every case exists value-free (unit weights) and weighted (weights that differ inside a forward row: the graph then leaves the
value-free kernels and the sweep, and serves the VF = false bodies of the binned and hub kernels).

Claims never depend on how the device orders rows of equal in-degree: a case is built from distinct degrees or from whole
slots of identically shaped rows wherever a claim hangs on which rows share a wave or a slot; the CPU test proves each claim
under the ascending and the descending order of equal degrees."""
import math

import numpy as np

from tests import chain_cases as cc

# the constants of spmv.hip / sweep.hip / build.hip the cases stand on (tests/test_spmv_cases.py reads them out of the sources)
EXPECTED_CONSTANTS = {"SW_GR": 4, "SW_G": 4, "SW_D": 16, "SW_MAXK": 4, "WPG": 8, "BN_MAX": 16384, "BN_STEP": 128,
                      "SWEEP_MIN_N": 50000, "HUB_T": 2048, "HUB_T_MIN": 128, "HS_R": 8, "HUB_PREFIX": 256, "HUB_GRID": 4096,
                      "BIN_WAVE": 128, "BIN_16": 32, "BIN_4": 4, "WAVE": 64}
WAVE = EXPECTED_CONSTANTS["WAVE"]
HS_PASS = WAVE * EXPECTED_CONSTANTS["HS_R"]
PREFIX = EXPECTED_CONSTANTS["HUB_PREFIX"]
BN_DEFAULT = EXPECTED_CONSTANTS["BN_MAX"]

NODE_USER, NODE_ITEM = 1, 2
D32 = float(np.float32(0.15))

# the knob sets: "default" runs in-process, every other one in a child process of its own (the library reads them once)
_SWEEP_CHILD = {"RWR_SWEEP_MIN_N": "0", "RWR_SWEEP_BN": "128", "RWR_HUB_T": "128"}
KNOBS = {
    "default": {},
    "phases": {"RWR_SPMV_PHASES": "1"},
    "hub128": {"RWR_HUB_T": "128"},
    "hub128_phases": {"RWR_HUB_T": "128", "RWR_SPMV_PHASES": "1"},
    "sweep_w1": dict(_SWEEP_CHILD, RWR_SWEEP_WGS="1"),
    "sweep_w3": dict(_SWEEP_CHILD, RWR_SWEEP_WGS="3"),
}


def knob_values(knobs):
    """(hub_t, BN, sweep_min_n, nwg or None, two-phase order) of a knob set, as the library resolves them"""
    env = KNOBS[knobs]
    hub_t = max(int(env.get("RWR_HUB_T", EXPECTED_CONSTANTS["HUB_T"])), EXPECTED_CONSTANTS["HUB_T_MIN"])
    bn = min(max(int(env.get("RWR_SWEEP_BN", BN_DEFAULT)), 128), BN_DEFAULT) & ~127
    wgs = int(env.get("RWR_SWEEP_WGS", 0))
    return hub_t, bn, int(env.get("RWR_SWEEP_MIN_N", EXPECTED_CONSTANTS["SWEEP_MIN_N"])), (wgs if wgs > 0 else None), \
        env.get("RWR_SPMV_PHASES") == "1"


class SpmvCase:
    """name, knobs (names in KNOBS), n, node_type, rows (j -> ascending int array of sources), seed, d, x, claims;
    flat(weighted) = the forward graph; the attributes tests/chain_cases.py's reference functions read are all here."""

    def __init__(self, name, knobs, n, node_type, rows, seed, x, claims, d=D32):
        self.name, self.knobs, self.n, self.node_type, self.seed, self.x, self.d = name, tuple(knobs), n, node_type, seed, x, d
        self.rows = {int(j): np.asarray(s, dtype=np.int64) for j, s in rows.items() if len(s)}
        for j, s in self.rows.items():
            assert (np.diff(s) >= 0).all() and s[0] >= 0 and s[-1] < n, (name, j)
        assert x.shape == (n,) and (x >= 0).all() and np.isfinite(x).all() and 0 <= seed < n
        self.claims = claims
        self._flat = {}
        self.in_deg = np.zeros(n, dtype=np.int64)
        for j, s in self.rows.items():
            self.in_deg[j] = len(s)

    def flat(self, weighted=False):
        if weighted not in self._flat:
            js = sorted(self.rows)
            in_src = np.concatenate([self.rows[j] for j in js]) if js else np.zeros(0, dtype=np.int64)
            in_dst = np.repeat(np.array(js, dtype=np.int64), [len(self.rows[j]) for j in js])
            order = np.argsort(in_src, kind="stable")            # forward lists: by source, targets ascending
            src = in_src[order]
            rowptr = np.zeros(self.n + 1, dtype=np.int64)
            rowptr[1:] = np.cumsum(np.bincount(src, minlength=self.n))
            m = len(src)
            pos = np.arange(m, dtype=np.int64) - rowptr[src]
            w = 1.0 + (pos % 3) if weighted else np.ones(m)
            self._flat[weighted] = dict(node_id=np.arange(self.n, dtype=np.int64) * 3 + 11, node_type=self.node_type.astype(np.uint8),
                                        rowptr=rowptr, dst=in_dst[order].astype(np.int32),
                                        etype=(1 + np.arange(m) % 7).astype(np.uint8), w=w.astype(np.float64))
        return self._flat[weighted]


# ---------------------------------------------------------------------------------------------------------- the reference

def normalised_fast(flat):
    """chain_cases.normalised for graphs whose links are all explicit and whose raw weights are small integers (every order
    of a row's weight sum is then exact): (w_norm per link, dangling per row)"""
    rowptr, w = flat["rowptr"], flat["w"]
    n = len(rowptr) - 1
    assert (flat["etype"] != 0).all() and (w == np.floor(w)).all() and w.max(initial=1.0) < 2.0 ** 20
    cnt = np.diff(rowptr)
    src = np.repeat(np.arange(n), cnt)
    sw = np.bincount(src, weights=w, minlength=n)
    return w / sw[src], cnt == 0


def _parts(case, weighted):
    """per link in IN-list order (by target, then source, then forward position -- the stable transpose of build.hip): the
    addend fl(fl((1 - d) x[src]) * w_norm); the in-list pointers; and the seed row's chain addends"""
    flat = case.flat(weighted)
    wn, dang = normalised_fast(flat)
    rowptr, dst = flat["rowptr"], flat["dst"].astype(np.int64)
    n = case.n
    src = np.repeat(np.arange(n), np.diff(rowptr))
    rw = (1 - case.d) * case.x                                   # Model.cs:84
    a_fwd = rw[src] * wn                                         # Model.cs:87
    order_in = np.argsort(dst, kind="stable")
    in_ptr = np.zeros(n + 1, dtype=np.int64)
    in_ptr[1:] = np.cumsum(np.bincount(dst, minlength=n))
    # the seed's row: per row in ascending order its links into the seed in list order, then its restart addend
    # (Model.cs:85-88, 91-93; a dangling row adds its whole rank, Model.cs:96-97)
    own = np.where(dang, case.x, case.x - rw)
    s0, s1 = int(in_ptr[case.seed]), int(in_ptr[case.seed + 1])
    seed_src = src[order_in[s0:s1]].tolist()
    seed_add = a_fwd[order_in[s0:s1]].tolist()
    chain, q = [], 0
    for i, o in enumerate(own.tolist()):
        while q < len(seed_src) and seed_src[q] == i:
            chain.append(seed_add[q])
            q += 1
        chain.append(o)
    assert q == len(seed_src)
    return a_fwd[order_in], in_ptr, src[order_in], chain


def reference(case, weighted=False):
    """Vectorised: round k adds the k-th in-link of every row that has one, which keeps every row's list order."""
    a_in, in_ptr, _, chain = _parts(case, weighted)
    deg = np.diff(in_ptr)
    by_deg = np.argsort(-deg, kind="stable")
    neg_sorted = -deg[by_deg]
    y = np.zeros(case.n, dtype=np.float64)
    for k in range(int(deg.max(initial=0))):
        rows = by_deg[:np.searchsorted(neg_sorted, -k, side="left")]      # the rows of more than k in-links
        y[rows] = y[rows] + a_in[in_ptr[rows] + k]
    y[case.seed] = cc.fold(chain)
    return y


def loop_reference(case, weighted=False, reverse_rows=()):
    """The plain loop: every row's in-list summed one by one (the rows of `reverse_rows` back to front)."""
    a_in, in_ptr, _, chain = _parts(case, weighted)
    a, p = a_in.tolist(), in_ptr.tolist()
    out = [0.0] * case.n
    for j in range(case.n):
        s = 0.0
        for v in (reversed(a[p[j]:p[j + 1]]) if j in reverse_rows else a[p[j]:p[j + 1]]):
            s = s + v
        out[j] = s
    out[case.seed] = cc.fold(chain)
    return np.array(out, dtype=np.float64)


# --------------------------------------------------------------------------------------------------------- building blocks

def noisy_x(rng, n):
    """mantissas of 52 random bits over 20 binades (wide enough that nearly every add rounds, narrow enough that no addend
    vanishes below the sum's last bit), a few zeros and subnormals: a wrong index, a swapped pair, a dropped or a doubled
    addend changes bits"""
    x = np.ldexp(1.0 + rng.random(n), rng.integers(-10, 10, n).astype(np.int32))
    x[rng.random(n) < 0.04] = 0.0
    sub = rng.random(n) < 0.01
    x[sub] = rng.integers(1, 1 << 30, int(sub.sum())) * 5e-324
    return x


def pick(rng, lo, hi, cnt, exclude=-1):
    """cnt distinct sources of [lo, hi), ascending, never `exclude`"""
    pool = np.arange(lo, hi)
    pool = pool[pool != exclude]
    assert cnt <= len(pool), (lo, hi, cnt)
    return np.sort(rng.choice(pool, size=cnt, replace=False))


def types_one(n):
    return np.full(n, NODE_USER, dtype=np.uint8)


def types_split(n):
    t = np.full(n, NODE_USER, dtype=np.uint8)
    t[n // 2:] = NODE_ITEM
    return t


def hub_passes(L):
    """k_spmv_exact_hub on a row of L in-links: (entries added one by one, passes of HS_PASS, entries of the last pass,
    the pipeline buffer -- 'a' or 'b' -- the last pass is folded from)"""
    pre = min(L, PREFIX)
    rest = L - pre
    passes = -(-rest // HS_PASS)
    return pre, passes, (rest - (passes - 1) * HS_PASS if passes else 0), ("-" if not passes else "ab"[(passes - 1) % 2])


# a row is named a target (its sum must depend on the order of its adds) from this many in-links on
MIN_TARGET = 5
DEG_ALL = [0, 1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 47, 48, 49, 127, 128, 129, 191, 192, 193, 255, 256, 257]


def _degree_case(name, knobs, rng, n, node_type, degs, seed_deg, claims, d=D32, pools=None, min_target=None):
    """rows of the in-degrees `degs` (one each, on scattered row ids), every other row without in-links; the seed is the row
    of in-degree seed_deg.  pools: per node type the [lo, hi) its rows draw their sources from (default: every node)."""
    ids = rng.permutation(n)[:len(degs)]
    rows = {}
    seed = None
    for j, L in zip(ids.tolist(), degs):
        lo, hi = (0, n) if pools is None else pools[int(node_type[j])]
        rows[j] = pick(rng, lo, hi, L, exclude=j)
        if L == seed_deg and seed is None:
            seed = j
    assert seed is not None
    claims = dict(claims, targets=sorted(j for j in rows if len(rows[j]) >= (min_target or MIN_TARGET) and j != seed))
    return SpmvCase(name, knobs, n, node_type, rows, seed, noisy_x(rng, n), claims, d)


# --------------------------------------------------------------------------------------------------------------- the cases

def _binned_cases(rng):
    out = []
    out.append(_degree_case("bins_every_degree_one_type", ["default"], rng, 1200, types_one(1200), DEG_ALL, 1, dict(
        kernel="binned", hub_launches=(0, 0), bins={"hub": 0, "wave": 8, "g16": 6, "g4": 9, "lane": 1177},
        mixed_wave=["g4"], partial_wave=["g16", "g4"], seed_body="lane",
        branch="every degree edge once, distinct degrees; the 4-lane body's one wave holds 4 and 31; seed in the lane body")))
    out.append(_degree_case("bins_every_degree_split", ["default", "phases"], rng, 1500, types_split(1500), DEG_ALL * 3, 9, dict(
        kernel="binned", hub_launches=(0, 0), bins={"hub": 0, "wave": 24, "g16": 18, "g4": 27, "lane": 1431},
        partial_wave=["g16", "g4"], seed_body="g4",
        branch="three rows of every degree over USER and ITEM rows, one- and two-phase order; seed in the 4-lane body")))
    out.append(_degree_case("bin16_shortest_and_longest_in_one_wave", ["default"], rng, 400, types_split(400), [127, 33, 32, 3, 1], 33, dict(
        kernel="binned", hub_launches=(0, 0), bins={"hub": 0, "wave": 0, "g16": 3, "g4": 0, "lane": 397},
        mixed_wave=["g16"], partial_wave=["g16"], seed_body="g16",
        branch="wave and 4-lane bins empty; the 16-lane body's one wave holds 127, 33 and 32 and one absent row; seed in it")))
    out.append(_degree_case("only_rows_of_at_most_3", ["default"], rng, 333, types_split(333), [3] * 40 + [2] * 30 + [1] * 50, 2, dict(
        kernel="binned", hub_launches=(0, 0), bins={"hub": 0, "wave": 0, "g16": 0, "g4": 0, "lane": 333}, seed_body="lane",
        branch="three bins empty: only rows of <= 3 in-links (two workgroups of the lane body)"), min_target=3))
    out.append(_degree_case("only_rows_of_at_least_128_and_of_0", ["default"], rng, 600, types_one(600), [128, 129, 191, 256, 257], 191, dict(
        kernel="binned", hub_launches=(0, 0), bins={"hub": 0, "wave": 5, "g16": 0, "g4": 0, "lane": 595}, seed_body="wave",
        branch="both group bins empty: rows of >= 128 and of 0 in-links only; 5 wave rows = a second workgroup of one wave; seed in the wave body")))
    out.append(_degree_case("no_4_lane_bin", ["default", "phases"], rng, 500, types_split(500), [0, 1, 3, 32, 48, 127, 128, 200, 3, 1], 48, dict(
        kernel="binned", hub_launches=(0, 0), bins={"hub": 0, "wave": 2, "g16": 3, "g4": 0, "lane": 495}, partial_wave=["g16"],
        seed_body="g16", branch="one bin empty (4 to 31 in-links)")))
    return out


def _hub_cases(rng):
    out = []
    p = PREFIX
    degs = [2047, 2048, 2049, p + 3 * HS_PASS, p + 3 * HS_PASS + 1, p + 4 * HS_PASS - 1, p + 4 * HS_PASS, p + 4 * HS_PASS + 1, 40, 5, 2]
    out.append(_degree_case("hub_default_threshold", ["default"], rng, 2500, types_split(2500), degs, 40, dict(
        kernel="binned", hub_launches=(1, 1), bins={"hub": 5, "wave": 3, "g16": 1, "g4": 1, "lane": 2490}, seed_body="g16", run_check=True,
        hub_rows={2048: (256, 4, 256, "b"), 2049: (256, 4, 257, "b"), p + 2047: (256, 4, 511, "b"), p + 2048: (256, 4, 512, "b"),
                  p + 2049: (256, 5, 1, "a")},
        branch="hub_t = 2048: 2047, p + 1536 and p + 1537 stay with the wave body (28 to 32 rounds of 64, the last partial); hub rows "
               "with last passes of 256, 257, 511, 512 and 1 entries")))
    out.append(_degree_case("hub_seed_is_a_hub_row", ["default"], rng, 2500, types_one(2500), [2100, 2060, 130, 6], 2100, dict(
        kernel="binned", hub_launches=(1, 1), bins={"hub": 2, "wave": 1, "g16": 0, "g4": 1, "lane": 2496}, seed_body="hub", run_check=True,
        hub_rows={2100: (256, 4, 308, "b"), 2060: (256, 4, 268, "b")},
        branch="the seed's row is a hub row: the hub kernel's `continue`; the chain writes it")))
    degs = [128, 255, 256, 257, p + 511, p + 512, p + 513, p + 1024, p + 1025, p + 1536, p + 1537, p + 2048 + 7, 127, 60, 9, 3]
    out.append(_degree_case("hub_passes_at_threshold_128", ["hub128"], rng, 2600, types_split(2600), degs, 60, dict(
        kernel="binned", hub_launches=(1, 1), bins={"hub": 12, "wave": 0, "g16": 2, "g4": 1, "lane": 2585}, seed_body="g16", run_check=True,
        hub_rows={128: (128, 0, 0, "-"), 255: (255, 0, 0, "-"), 256: (256, 0, 0, "-"), 257: (256, 1, 1, "a"), p + 511: (256, 1, 511, "a"),
                  p + 512: (256, 1, 512, "a"), p + 513: (256, 2, 1, "b"), p + 1024: (256, 2, 512, "b"), p + 1025: (256, 3, 1, "a"),
                  p + 1536: (256, 3, 512, "a"), p + 1537: (256, 4, 1, "b"), p + 2055: (256, 5, 7, "a")},
        branch="hub_t = 128: zero to five passes, every pipeline buffer the last one, last passes of 1, 7, 511 (not multiples of 8) and 512")))
    # more hub rows than the hub kernel's grid: rows of exactly 128 in-links, all in the prefix
    n = 4300
    ids = rng.permutation(n)[:EXPECTED_CONSTANTS["HUB_GRID"] + 1]
    rows = {int(j): pick(rng, 0, n, 128, exclude=int(j)) for j in ids}
    out.append(SpmvCase("hub_grid_stride", ["hub128"], n, types_split(n), rows, int(ids[7]), noisy_x(rng, n), dict(
        kernel="binned", hub_launches=(1, 1), bins={"hub": 4097, "wave": 0, "g16": 0, "g4": 0, "lane": 203}, seed_body="hub", run_check=True,
        targets=[int(j) for j in ids[:40] if j != ids[7]], hub_rows={128: (128, 0, 0, "-")},
        branch="4097 hub rows of 128 in-links: the grid of 4096 strides once; the seed is one of them")))
    # hub rows by phase (two-phase order): ITEM rows only, the other rows only, both
    for name, want, launches in (("hub_rows_item_phase_only", [NODE_ITEM], 1), ("hub_rows_other_phase_only", [NODE_USER], 1),
                                 ("hub_rows_both_phases", [NODE_ITEM, NODE_USER], 2)):
        n = 900
        t = types_split(n)
        hubs = [int(j) for ty in want for j in rng.permutation(np.nonzero(t == ty)[0])[:3]]
        rows = {j: pick(rng, 0, n, L, exclude=j) for j, L in zip(hubs, [300, 770, 129, 769, 131, 257])}
        others = [int(j) for j in rng.permutation(n)[:40] if j not in rows]
        rows.update({j: pick(rng, 0, n, L, exclude=j) for j, L in zip(others, [100, 50, 20, 7, 3, 1] * 6)})
        out.append(SpmvCase(name, ["hub128_phases"], n, t, rows, others[1], noisy_x(rng, n), dict(
            kernel="binned", hub_launches=(launches, launches), run_check=True, targets=hubs, hub_types=want,
            branch="two-phase order, hub rows in " + " and ".join("ITEM" if ty == NODE_ITEM else "USER" for ty in want) + " rows")))
    # the chain cases' value pattern on one hub row: noisy head, level to 1.5 * 2^E, then half-ulp fillers, zeros and subnormals.
    # d = 0.5 and sources of exactly one link each: the addends are exactly x / 2
    n, L = 2300, PREFIX + 2 * HS_PASS + 300
    hub = 2222
    srcs = np.arange(100, 100 + L)
    x = noisy_x(rng, n)
    s, seq = 0.0, []
    for a in cc.noisy(rng, 200):
        seq.append(a)
        s = s + a
    m, e = math.frexp(s)
    T = math.ldexp(0.75, e) if m <= 0.75 else math.ldexp(1.5, e)
    seq.append(T - s)
    u = math.ldexp(1.0, (e - 1 if m <= 0.75 else e) - 52)
    fill = cc.filler(rng, L - len(seq), u)
    for q in range(0, len(fill), 37):
        fill[q] = float(rng.integers(1, 1 << 20)) * 5e-324
    seq += fill
    x[srcs] = 2.0 * np.array(seq)
    assert cc.fold(seq[:201]) == T and (x[srcs] * 0.5 == np.array(seq)).all()
    rows = {hub: srcs, 2250: pick(rng, 0, 100, 60), 2251: pick(rng, 0, 100, 5)}
    out.append(SpmvCase("hub_level_then_half_ulp_fillers", ["hub128"], n, types_split(n), rows, 2250, x, dict(
        kernel="binned", hub_launches=(1, 1), targets=[hub], run_check=True, hub_rows={L: (256, 3, 300, "a")}, exact_addends=hub, frozen=set(srcs.tolist()),
        branch="hub row: head, a sum levelled to 1.5 * 2^E inside the prefix, then ties, near-ties, zeros and subnormals through the exact fold"), d=0.5))
    return out


def _sweep_default_cases(rng):
    """n >= 50 000 at default knobs: the geometry follows the CU count, so only what holds for every geometry is claimed"""
    out = []
    BN = BN_DEFAULT
    for n in (65535, 65536, 65537, 65538, 4 * BN + 127, 4 * BN + 128, 4 * BN + 129):
        t = types_split(n)
        rows = {}
        ids = rng.permutation(n)
        body = ids[:24000]                                        # short rows all over the vector
        for j, L in zip(body.tolist(), rng.integers(1, 9, len(body)).tolist()):
            rows[j] = pick_sparse(rng, n, L, j)
        edge = [int(j) for j in ids[24000:24012]]
        ends = np.array([BN - 1, BN, 2 * BN - 1, 2 * BN, 3 * BN - 1, 3 * BN, 4 * BN - 1] + ([4 * BN] if n > 4 * BN + 3 else []) + [n - 3, n - 2, n - 1])
        for q, j in enumerate(edge):                              # pieces that split at every block edge; links out of n-3 .. n-1
            extra = pick_sparse(rng, n, 5 + q, j)
            rows[j] = np.unique(np.concatenate([ends[(ends != j) & (ends < n)], extra]))
        long_rows = [int(j) for j in ids[24012:24015]]
        for q, j in enumerate(long_rows):                         # 2047 in-links out of ONE block: the longest piece there is
            rows[j] = pick(rng, q * BN, (q + 1) * BN, 2047, exclude=j)
        hub = int(ids[24015])
        rows[hub] = pick(rng, 0, n, 2500, exclude=hub)
        seed = edge[3]
        out.append(SpmvCase(f"sweep_n{n}", ["default"], n, t, rows, seed, noisy_x(rng, n), dict(
            kernel="sweep", hub_launches=(1, 1), targets=[j for j in edge if j != seed] + long_rows + [hub], run_check=True, reads_last=edge, n_tail=n % BN,
            features=["piece_ge_40", "seed_in_sweep"] + (["n_sw_not_mult_64"] if (n - 1) % 64 else []),
            branch=f"n = {n}: last block of {n % BN or BN}; rows reading z[n-3 .. n-1] and both sides of every block edge; "
                   "2047-entry pieces; one hub row beside the sweep")))
    return out


def pick_sparse(rng, n, cnt, exclude):
    s = np.unique(rng.integers(0, n, cnt + 2))
    return s[s != exclude][:cnt]


def _slot_case(name, knobs, rng, n, node_type, slots, claims, lone=(), seed_slot=0, hubs=()):
    """slots: per slot the pieces {block: entries} shared by its 64 rows (in-degrees must fall from slot to slot, so that the
    in-degree order IS the slot order whatever the order of equal degrees); lone: rows of their own, (pieces, count) each --
    they join the next slot down the order; hubs: in-degrees of hub rows.  Row ids are scattered; BN = 128."""
    ids = [int(v) for v in rng.permutation(n)]
    rows, targets = {}, []
    seed = None

    def make(j, pieces):
        parts = []
        for b in sorted(pieces):
            spec = pieces[b]
            parts.append(np.asarray(spec) if not isinstance(spec, int) else pick(rng, b * 128, min(n, (b + 1) * 128), spec, exclude=j))
        rows[j] = np.concatenate(parts)

    for k, pieces in enumerate(slots):
        for q in range(64):
            j = ids.pop()
            make(j, pieces)
            if q == 0:
                targets.append(j)
            if k == seed_slot and q == 5:
                seed = j
    for pieces, count in lone:
        for q in range(count):
            j = ids.pop()
            make(j, pieces)
            if q == 0:
                targets.append(j)
    for L in hubs:
        j = ids.pop()
        rows[j] = pick(rng, 0, n, L, exclude=j)
        targets.append(j)
    claims = dict(claims, targets=[j for j in targets if len(rows.get(j, ())) >= MIN_TARGET and j != seed], kernel="sweep", run_check=True)
    return SpmvCase(name, knobs, n, node_type, rows, seed, noisy_x(rng, n), claims)


def _sweep_child_cases(rng):
    out = []
    # --- K = 1, one workgroup: 8 slots = 8 waves, one stream each.  385 nodes: the last block holds ONE element and n is odd
    n = 385
    slots = [
        {0: 40, 1: 40, 2: 24, 3: [n - 1]},                         # 10 + 10 + 6 + 1 = 27 word-rows
        {0: 16, 1: 17, 2: 22, 3: [n - 1]},                         # 4 + 5 + 6 + 1: pieces end on, behind and before a group boundary
        {1: 4, 2: 5},                                              # an empty piece in visited block 0, and in 3: the stream's last
        {0: 1, 1: 2, 2: 3, 3: [n - 1]},                            # four pieces of one word-row in one group (1, 2, 3, 1 entries)
        {2: 6},                                                    # two empty pieces in a row, 6 entries = 2 word-rows
    ]
    out.append(_slot_case("sweep_k1_last_block_of_1_odd_n", ["sweep_w1"], rng, n, types_one(n), slots, dict(
        hub_launches=(0, 0), geometry=dict(k=1, blocks=4, wgs=1, partial=0), T=[27, 16, 3, 4, 2, 0, 0, 0],
        features=["last_pair_prev_block", "last_block_elems:1", "end_on_group", "end_after_group", "end_before_group",
                  "three_pieces_in_group", "empty_piece_visited", "two_empty_in_row", "empty_last", "n_sw_not_mult_64", "seed_in_sweep",
                  "word_padding:1", "word_padding:2", "word_padding:3", "word_padding:4", "word_padding:5", "T:0", "T:3", "T:4", "T:16"],
        reads_last=True, branch="K = 1; n odd and the last block one element (last_pair in the previous block); piece ends on / "
                                "behind / before a group boundary; one-word pieces; empty pieces; T = 0 for the waves of the rows without in-links")))
    # --- K = 1, three workgroups: 24 streams, the stream lengths around the rolling prefetch's depth; block 2 read by slot 0's
    #     workgroup only; n = 6 * 128 + 2.  Pieces of wr word-rows hold 4 wr - 3 entries, which keeps 34 word-rows under hub_t = 128
    n = 770
    slots = []
    for T in [33, 32, 31, 17, 16, 15, 5, 4, 3, 1]:
        pieces, left = {}, T
        for b in (0, 1, 3, 4, 5):
            wr = min(left, 7)
            if wr:
                pieces[b] = 4 * wr - 3
            left -= wr
        assert left == 0
        slots.append(pieces)
    slots[0][2] = [256 + 3, 256 + 77]                              # 33 -> 34 word-rows for slot 0, the only reader of block 2
    # three rows of 4 in-links: they share a slot with 61 of the one-link rows (unequal pieces: row padding; 2 word-rows), and
    # push the last 3 one-link rows into a slot of their own (1 word-row)
    lone = [({0: [5, 9], 6: [n - 2, n - 1]}, 3)]
    out.append(_slot_case("sweep_k1_three_workgroups_stream_lengths", ["sweep_w3"], rng, n, types_one(n), slots, dict(
        hub_launches=(0, 0), geometry=dict(k=1, blocks=7, wgs=3, partial=0), T=[34, 32, 31, 17, 16, 15, 5, 4, 3, 2, 1] + [0] * 13,
        features=["T:0", "T:1", "T:3", "T:4", "T:5", "T:15", "T:16", "T:17", "T:31", "T:32", "wg_skips_block", "row_padding",
                  "last_block_elems:2", "seed_in_sweep", "n_sw_not_mult_64"],
        reads_last=True, branch="K = 1 on 3 workgroups: streams of 0, 1, 3, 4, 5, 15, 16, 17, 31, 32 word-rows; a workgroup that skips "
                                "a block between two it visits; a slot of unequal rows (row padding); last block of 2"), lone=lone))
    # --- T = 33 on one workgroup (a stream one word-row longer than two prefetch rounds), K = 1, n = 4 * 128: the last block full
    n = 512
    slots = [{0: 36, 1: 36, 2: 36, 3: 19}, {0: 9, 3: [n - 3, n - 2, n - 1]}]
    out.append(_slot_case("sweep_k1_stream_of_33_last_block_full", ["sweep_w1"], rng, n, types_one(n), slots, dict(
        hub_launches=(0, 0), geometry=dict(k=1, blocks=4, wgs=1, partial=0), T=[32, 4, 0, 0, 0, 0, 0, 0],
        features=["T:32", "last_block_elems:128", "seed_in_sweep"], reads_last=True,
        branch="K = 1, n = B * BN exactly (n_sw a multiple of 64); links out of n-3, n-2, n-1")))
    n = 512
    slots = [{0: 33, 1: 33, 2: 33, 3: 21}, {0: 9, 3: [n - 3, n - 2, n - 1]}]
    out.append(_slot_case("sweep_k1_stream_of_33", ["sweep_w1"], rng, n, types_one(n), slots, dict(
        hub_launches=(0, 0), geometry=dict(k=1, blocks=4, wgs=1, partial=0), T=[33, 4, 0, 0, 0, 0, 0, 0],
        features=["T:33", "seed_in_sweep"], reads_last=True, branch="K = 1: a stream of 33 word-rows")))
    # --- K = 2, 3, 4 by row count alone (one workgroup), with a hub row beside the sweep; last blocks of 2, 127 and 128
    for K, n in ((2, 7 * 128 + 2), (3, 10 * 128 + 127), (4, 16 * 128)):
        B = -(-n // 128)
        slots = []
        for k in range(8 * (K - 1) + 3):                           # the last of the K slots of most waves: rows without in-links
            b0 = k % (B - 1)
            slots.append({b0: 30 - (k % 23), (b0 + 2) % (B - 1): 1 + k % 5, B - 1: [n - 1] if k % 3 else [n - 2, n - 1]})
        slots.sort(key=lambda p: -sum(v if isinstance(v, int) else len(v) for v in p.values()))
        degs = [sum(v if isinstance(v, int) else len(v) for v in p.values()) for p in slots]
        for k in range(1, len(slots)):                             # strictly falling in-degrees from slot to slot
            while degs[k] >= degs[k - 1]:
                b0 = min(b for b in slots[k] if isinstance(slots[k][b], int) and slots[k][b] > 1)
                slots[k][b0] -= 1
                degs[k] -= 1
        out.append(_slot_case(f"sweep_k{K}_by_row_count", ["sweep_w1"], rng, n, types_split(n), slots, dict(
            hub_launches=(1, 1), geometry=dict(k=K, blocks=B, wgs=1, partial=0),
            features=["seed_in_sweep", f"last_block_elems:{n - (B - 1) * 128}", "empty_piece_visited"], reads_last=True,
            branch=f"K = {K}: {n} rows on one workgroup; one hub row on its own stream beside the sweep"), hubs=[300], seed_slot=9 if K > 2 else 2))
    # --- few rows on three workgroups: workgroup 2 owns no entries at all (nb = 0, T = 0) and still writes its +0.0 rows
    n = 3 * 128 + 3
    slots = [{0: 20, 1: 7, 3: [n - 1]}, {1: 9, 3: [n - 3, n - 2]}]
    out.append(_slot_case("sweep_workgroup_without_entries", ["sweep_w3"], rng, n, types_one(n), slots, dict(
        hub_launches=(0, 0), geometry=dict(k=1, blocks=4, wgs=3, partial=0), features=["wg_no_entries", "last_block_elems:3", "seed_in_sweep"],
        reads_last=True, branch="3 workgroups, entries in the slots of two: the third has nb = 0 and T = 0")))
    # --- more than 2048 non-hub rows on one workgroup: the ITEM rows alone (phase 0), the other rows on the row-binned kernel beside
    #     the sweep; the ITEM rows read 12 of the 21 blocks.  n = 20 * 128 + 3
    n = 20 * 128 + 3
    t = np.full(n, NODE_USER, dtype=np.uint8)
    t[:600] = NODE_ITEM
    rows = {}
    items = rng.permutation(600)
    for q, j in enumerate(items[:400].tolist()):
        L = 1 + q % 90
        rows[j] = np.unique(np.concatenate([pick(rng, 640, 2048, L), [n - 1 - q % 3]]))
    rows[int(items[400])] = pick(rng, 640, 2048, 200)               # a hub row among the ITEM rows
    users = 600 + rng.permutation(n - 600)
    for q, j in enumerate(users[:900].tolist()):
        rows[j] = pick(rng, 0, 600, 1 + q % 120)
    rows[int(users[900])] = pick(rng, 0, 600, 333)                  # ... and one among the others
    targets = [int(j) for j in items[5:400:37]] + [int(items[400]), int(users[5]), int(users[900])]
    assert all(len(rows[j]) >= MIN_TARGET for j in targets)
    out.append(SpmvCase("sweep_item_rows_only", ["sweep_w1"], n, t, rows, int(items[44]), noisy_x(rng, n), dict(
        kernel="sweep", run_check=True, hub_launches=(2, 1), binned_beside=True, geometry=dict(k=2, blocks=21, wgs=1, partial=1),
        targets=targets, features=["wg_skips_block", "seed_in_sweep", "last_block_elems:3", "n_sw_not_mult_64"], reads_last=True,
        branch="ITEM-rows-only form: 2562 non-hub rows on one workgroup; a hub row in each phase; the ITEM rows skip blocks 0-4 and 16-19")))
    return out


def _sensitise(case, rng):
    """Every target row's sum must depend on the order of its adds, in both forms (a kernel that reassociated the row, or
    walked it from the wrong end, must not pass).  A sum of a few dozen random addends survives a reversal in roughly one case
    out of five, so: while the back-to-front sum of a target equals its list-order sum, one of its sources draws a new rank --
    one that leaves every other target that reads this source order-dependent."""
    frozen = case.claims.get("frozen", set())
    c1 = 1 - case.d
    forms = []
    for weighted in (False, True):
        flat = case.flat(weighted)
        wn, _ = normalised_fast(flat)
        order_in = np.argsort(flat["dst"], kind="stable")
        in_ptr = np.zeros(case.n + 1, dtype=np.int64)
        in_ptr[1:] = np.cumsum(np.bincount(flat["dst"], minlength=case.n))
        forms.append((in_ptr, np.repeat(np.arange(case.n), np.diff(flat["rowptr"]))[order_in], wn[order_in]))

    def ok(j):
        for in_ptr, src_in, wn_in in forms:
            seg = ((c1 * case.x[src_in[in_ptr[j]:in_ptr[j + 1]]]) * wn_in[in_ptr[j]:in_ptr[j + 1]]).tolist()
            if cc.fold(seg) == cc.fold(reversed(seg)):
                return False
        return True

    targets = case.claims["targets"]
    readers = {}
    for j in targets:
        for u in case.rows[j].tolist():
            readers.setdefault(u, []).append(j)
    for j in list(targets):
        if ok(j):
            continue
        srcs = [u for u in case.rows[j].tolist() if u not in frozen]
        assert srcs, (case.name, j)
        for _ in range(300):
            u = srcs[int(rng.integers(len(srcs)))]
            keep = [t for t in readers[u] if t != j and ok(t)]
            old = case.x[u]
            case.x[u] = math.ldexp(1.0 + rng.random(), int(rng.integers(-10, 10)))
            if ok(j) and all(ok(t) for t in keep):
                break
            case.x[u] = old
        else:
            # (three addends rarely round differently back to front: such a row is then not named a target)
            assert len(case.rows[j]) < MIN_TARGET, (case.name, j)
            case.claims["targets"] = [t for t in case.claims["targets"] if t != j]
    targets = case.claims["targets"]
    assert targets and all(ok(j) for j in targets), case.name
    return case


def make_cases():
    rng = np.random.default_rng(20240919)
    return [_sensitise(c, rng) for c in _binned_cases(rng) + _hub_cases(rng) + _sweep_default_cases(rng) + _sweep_child_cases(rng)]


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = make_cases()
    return _CASES


def cases_for(knobs):
    return [c for c in cases() if knobs in c.knobs]
