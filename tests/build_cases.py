"""Crafted graphs for the device-side graph build (build.hip: row_prepare_body, k_in_ptr, k_gather_in, the order-key kernels,
k_build_small; sort.hip; sort_small.h), one named case per decision point of that code, with a model of the layout the build
chooses and plain list-order references in double precision.  Pure Python / numpy: no GPU import.
tests/test_build_cases.py proves every case's claims on the CPU, tests/test_gpu_build_edges.py and tests/build_edges_child.py
run the cases.

A case is a flat graph (the arrays of include/rwr.h), one or two weight forms ("weighted": crafted weights, the graph is not
uniform and the step reads in_w; "uniform": every row's explicit weights equal, the step reads w_src on the value-free path),
a rank vector x >= 0, d = 0.5, a seed and a dict of claims.  Claims name positions: `rows` are the source rows whose weight
sum must depend on how the row pass walks them (per row: the places inside the row where a tile edge falls), `in_rows` the
target rows whose in-list order must show in one Model.deliverRanks.  Those positions carry planted values: a row named in
`rows` is redrawn until every mutant of the row pass changes its w_norm bits; a row named in `in_rows` takes its links from
single-link source rows (w_norm exactly 1, d = 0.5: the addend is exactly x / 2) whose ranks spell one large addend followed
by addends of half an ulp to a few ulps, chosen so that every swap of two neighbours changes the sum's bits."""
import numpy as np

EXPECTED_CONSTANTS = {"RP_CAP": 2048, "RP_WPB": 4, "BS_CAP": 1024, "BS_ROW_WAVES": 8, "ONE_LAUNCH_MAX_N": 8192,
                      "ONE_LAUNCH_MAX_M": 65536, "SMALL_SORT_MAX": 20480, "SMALL_SORT_THREADS": 1024, "SORT_BLOCK": 256,
                      "SORT_ITEMS": 16, "WAVE": 64}
K_ = EXPECTED_CONSTANTS
WAVE = K_["WAVE"]
MAXN, MAXM = K_["ONE_LAUNCH_MAX_N"], K_["ONE_LAUNCH_MAX_M"]
SORT_CHUNK = K_["SORT_BLOCK"] * K_["SORT_ITEMS"]
SMALL_WAVES = K_["SMALL_SORT_THREADS"] // WAVE
NODE_USER, NODE_ITEM = 1, 2
EDGE_UNDEFINED, EDGE_LIKE, EDGE_FRIENDSHIP = 0, 1, 2
D = 0.5
U = 2.0 ** -52
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def fold(seq, s=0.0):
    for a in seq:
        s = s + a
    return s


# ------------------------------------------------------------------------------------------------------ the layout model

def bit_length(v):
    return int(v).bit_length()


def key_bits(top):
    return max(1, bit_length(top))


def one_launch(n, m):
    """graph_fits_small_build: the shipped library reads no knob, sizes alone choose the build"""
    return 0 < n <= MAXN and 0 <= m <= MAXM


def tile_cap(n, m):
    return K_["BS_CAP"] if one_launch(n, m) else K_["RP_CAP"]


def groups(n, m, rowptr):
    """per 64-row group: (L0, L1, branch) -- 'long' iff the group holds more than 8 * CAP links, else 'tiled'"""
    cap = tile_cap(n, m)
    out = []
    for r0 in range(0, n, WAVE):
        L0, L1 = int(rowptr[r0]), int(rowptr[min(n, r0 + WAVE)])
        out.append((L0, L1, "long" if L1 - L0 > 8 * cap else "tiled"))
    return out


def link_place(n, m, rowptr, q):
    """(group, tile, offset in the tile, sweep-2 lane) of raw link q"""
    row = int(np.searchsorted(rowptr, q, side="right")) - 1
    g = row // WAVE
    L0 = int(rowptr[g * WAVE])
    cap = tile_cap(n, m)
    return g, (q - L0) // cap, (q - L0) % cap, (q - L0) % WAVE


def row_edges(n, m, rowptr, i):
    """the places k (0 < k < length) inside row i where a tile edge falls; [] in the long-row branch, which has no tiles"""
    g = i // WAVE
    L0, L1, branch = groups(n, m, rowptr)[g]
    if branch == "long":
        return []
    cap = tile_cap(n, m)
    b, e = int(rowptr[i]), int(rowptr[i + 1])
    return [T - b for T in range(L0 + cap, L1, cap) if b < T < e]


def serving_wave(n, m, i):
    """one-launch build: (wave, turn) that serves row i's group -- turn >= 1 reuses the wave's LDS arrays"""
    g = i // WAVE
    return (g % K_["BS_ROW_WAVES"], g // K_["BS_ROW_WAVES"]) if one_launch(n, m) else (g % K_["RP_WPB"], 0)


def sort_form(one, count, bits_):
    """(form, passes, blocks, result in the alternate buffer) of one radix sort of `count` keys of `bits_` bits"""
    if count == 0:
        return ("none", 0, 0, False)
    passes = (bits_ + 7) // 8
    if one:
        return ("body", passes, 1, bool(passes & 1))
    if count <= K_["SMALL_SORT_MAX"]:
        return ("small", passes, 1, bool(passes & 1))
    return ("multi", passes, -(-count // SORT_CHUNK), bool(passes & 1))


def orderable(v):
    return (int(v) + (1 << 63)) & ((1 << 64) - 1)


def sort_plan(n, m, nnz, max_in_deg, item_ids):
    """the five sorts of a first build"""
    one = one_launch(n, m)
    n_items = len(item_ids)
    span = (max(orderable(v) for v in item_ids) - min(orderable(v) for v in item_ids)) if n_items else 0
    top_bits = key_bits(nnz)
    return {
        "links": sort_form(one, m, bit_length(n)),
        "row_order": sort_form(one, n, key_bits(max_in_deg) if one else top_bits),
        "row_order_x": sort_form(one, n, 1 if one else min(top_bits, 31) + 1),
        "item_rows": sort_form(one, n, 8),
        "item_order": sort_form(one, n_items, key_bits(span) if n_items else 1),
    }


def sort_ranges(form, count):
    """the contiguous key ranges whose order a stable sort of that form has to stitch: waves (one workgroup) or blocks"""
    if form[0] == "multi":
        return [(b * SORT_CHUNK, min(count, (b + 1) * SORT_CHUNK)) for b in range(form[2])]
    per = -(-(-(-count // SMALL_WAVES)) // WAVE) * WAVE
    return [(min(count, w * per), min(count, (w + 1) * per)) for w in range(SMALL_WAVES)]


# --------------------------------------------------------------------------------------------------------- the references

def normalise(flat, w=None):
    """Graph.buildGraph (Graph.cs:51-88) in strict list order: dict(w_norm, dangling, uniform, nonneg, nnz)"""
    rowptr, et = flat["rowptr"], flat["etype"]
    w = flat["w"] if w is None else w
    n, m = len(rowptr) - 1, len(w)
    wl, ex = w.tolist(), (et != EDGE_UNDEFINED).tolist()
    rp = rowptr.tolist()
    wn = [0.0] * m
    dang = np.ones(n, dtype=np.uint8)
    uniform, nonneg = True, True
    for i in np.nonzero(np.diff(rowptr))[0].tolist():
        s, first, cnt = 0.0, None, 0
        for p in range(rp[i], rp[i + 1]):
            if ex[p]:
                v = wl[p]
                if cnt == 0:
                    first = v
                elif v != first:
                    uniform = False
                s = s + v
                cnt += 1
                if not v >= 0.0:
                    nonneg = False
        if cnt:
            dang[i] = 0
            if not (0.0 < s < float("inf")):
                nonneg = False
            with np.errstate(all="ignore"):
                q = (np.array(wl[rp[i]:rp[i + 1]]) / s).tolist()       # IEEE divide (Graph.cs:81)
            for p in range(rp[i], rp[i + 1]):
                if ex[p]:
                    wn[p] = q[p - rp[i]]
    return dict(w_norm=np.array(wn, dtype=np.float64), dangling=dang, uniform=int(uniform), nonneg=int(nonneg),
                uniform_path=int(uniform and nonneg), nnz=int(sum(ex)))


def in_lists(flat, w_norm, x, d=D):
    """the stable transpose: per explicit link in (target, source ascending, list position ascending) order its addend
    fl(fl((1 - d) x[u]) * w), its source and its raw position; and in_ptr"""
    rowptr, dst, et = flat["rowptr"], flat["dst"].astype(np.int64), flat["etype"]
    n = len(rowptr) - 1
    src = np.repeat(np.arange(n), np.diff(rowptr))
    keep = np.nonzero(et != EDGE_UNDEFINED)[0]
    order = keep[np.argsort(dst[keep], kind="stable")]
    with np.errstate(all="ignore"):
        add = (((1 - d) * x)[src[order]]) * w_norm[order]          # Model.cs:84,87
    in_ptr = np.zeros(n + 1, dtype=np.int64)
    in_ptr[1:] = np.cumsum(np.bincount(dst[keep], minlength=n))
    return add, src[order], order, in_ptr


def deliver_reference(flat, norm, x, seed, d=D):
    """one Model.deliverRanks (Model.cs:76-100) on rank = x of the seed's model: nextRank[j] is the left fold of the in-links'
    addends; the seed's row takes, row by row in ascending order, the row's links into the seed and then its restart addend"""
    n = len(flat["rowptr"]) - 1
    add, src_in, _, in_ptr = in_lists(flat, norm["w_norm"], x, d)
    deg = np.diff(in_ptr)
    by_deg = np.argsort(-deg, kind="stable")
    neg_sorted = -deg[by_deg]
    y = np.zeros(n, dtype=np.float64)
    with np.errstate(all="ignore"):
        for k in range(int(deg.max(initial=0))):                   # round k adds every row's k-th in-link: list order per row
            rows = by_deg[:np.searchsorted(neg_sorted, -k, side="left")]
            y[rows] = y[rows] + add[in_ptr[rows] + k]
    rw = (1 - d) * x
    own = np.where(norm["dangling"] != 0, x, x - rw).tolist()      # Model.cs:91-93, 96-97
    s0, s1 = int(in_ptr[seed]), int(in_ptr[seed + 1])
    ssrc, sadd = src_in[s0:s1].tolist(), add[s0:s1].tolist()
    s, q = 0.0, 0
    for i in range(n):
        while q < len(ssrc) and ssrc[q] == i:
            s = s + sadd[q]
            q += 1
        s = s + own[i]
    y[seed] = s
    return y


def loop_in_row(flat, norm, x, j, d=D):
    """row j's in-link addends (list order), their sources and raw positions: the plain form the mutants work on"""
    add, src_in, order, in_ptr = in_lists(flat, norm["w_norm"], x, d)
    a, b = int(in_ptr[j]), int(in_ptr[j + 1])
    return add[a:b].tolist(), src_in[a:b].tolist(), order[a:b].tolist()


def ranked_all_ties(flat, norm, seed, top_n):
    """Recommendation of a DANGLING seed (all its rank returns to it: every other score is +0.0): the seed first if it is an
    ITEM, then the items by id descending, less the targets of the seed's LIKE links (Recommender.cs:20-38)"""
    assert norm["dangling"][seed]
    rowptr, dst, et = flat["rowptr"], flat["dst"], flat["etype"]
    excl = {int(dst[p]) for p in range(int(rowptr[seed]), int(rowptr[seed + 1])) if et[p] == EDGE_LIKE}
    items = [i for i in np.nonzero(flat["node_type"] == NODE_ITEM)[0].tolist() if i not in excl]
    items.sort(key=lambda i: -int(flat["node_id"][i]))
    if flat["node_type"][seed] == NODE_ITEM and seed not in excl:
        items = [seed] + [i for i in items if i != seed]
    return [int(flat["node_id"][i]) for i in items[:top_n]]


# ------------------------------------------------------------------------------------------- the mutants of the row pass

def pairwise8(v):
    s = 0.0
    for c in range(0, len(v), 8):
        t = list(v[c:c + 8])
        while len(t) > 1:
            t = [t[i] + t[i + 1] if i + 1 < len(t) else t[i] for i in range(0, len(t), 2)]
        s = s + t[0]
    return s


def row_mutant_sums(ws, ex, edges):
    """{mutant name: the row's weight sum under it}; ws / ex = the row's raw weights and which are explicit; edges = the
    places inside the row.  'drop' / 'double' act on the nearest explicit entry on each side of an edge."""
    L = len(ws)
    v = [ws[p] for p in range(L) if ex[p]]
    out = {"pairwise8": pairwise8(v)}
    for k in edges:
        ke = sum(ex[:k])
        assert 0 < ke < len(v), "an edge needs explicit entries on both sides"
        out[f"restart@{k}"] = fold(v[ke:])
        out[f"drop_before@{k}"] = fold(v[:ke - 1] + v[ke:])
        out[f"drop_after@{k}"] = fold(v[:ke] + v[ke + 1:])
        out[f"double_before@{k}"] = fold(v[:ke] + [v[ke - 1]] + v[ke:])
        out[f"double_after@{k}"] = fold(v[:ke + 1] + [v[ke]] + v[ke + 1:])
    cuts = [0] + [sum(ex[:k]) for k in edges] + [len(v)]
    if edges:
        out["partial_sums"] = fold([fold(v[cuts[t]:cuts[t + 1]]) for t in range(len(cuts) - 1)])
    return out


def mutant_edges(case, i):
    """the places a named row's mutants cut at: its tile edges, or (long-row branch: no tiles) the 8-entry batch edge nearest
    its middle"""
    f = case.flat
    n, m = case.n, case.m
    e = row_edges(n, m, f["rowptr"], i)
    if e:
        return e
    L = int(f["rowptr"][i + 1] - f["rowptr"][i])
    return [8 * max(1, L // 16)] if L > 8 else []


def row_survivors(case, i, w):
    """the mutants that leave row i's w_norm bits unchanged (must be none for a named row)"""
    f = case.flat
    b, e = int(f["rowptr"][i]), int(f["rowptr"][i + 1])
    ws, ex = w[b:e].tolist(), (f["etype"][b:e] != EDGE_UNDEFINED).tolist()
    v = np.array([ws[p] for p in range(e - b) if ex[p]])
    s = fold(v.tolist())
    return [k for k, t in row_mutant_sums(ws, ex, mutant_edges(case, i)).items() if (bits(v / t) == bits(v / s)).all()]


def in_row_survivors(case, j, form):
    """the transpose mutants that leave row j's nextRank bits unchanged: 'swap@k' exchanges in-links k and k + 1 (k >= 1: the
    first two addends meet in one commutative add, no order of them can show), 'src-1@k' / 'src+1@k' attribute in-link k to
    the neighbouring source row"""
    f, x = case.flat, case.x
    norm = case.norm(form)
    a, srcs, pos = loop_in_row(f, norm, x, j)
    base, out = fold(a), []
    for k in range(1, len(a) - 1):
        t = list(a)
        t[k], t[k + 1] = t[k + 1], t[k]
        if fold(t) == base:
            out.append(f"swap@{k}")
    for k in range(len(a)):
        for dlt in (-1, 1):
            u = srcs[k] + dlt
            if 0 <= u < case.n:
                t = list(a)
                t[k] = ((1 - D) * float(x[u])) * float(norm["w_norm"][pos[k]])
                if fold(t) == base:
                    out.append(f"src{dlt:+d}@{k}")
    return out


# ------------------------------------------------------------------------------------------------------------ building

def craft_sequence(rng, L):
    """one large addend, then addends of half an ulp to a few ulps of it, such that swapping ANY two neighbours (from the second
    on) changes the left fold's bits.  Grown one addend at a time: mut[i] is the running sum with the neighbours i, i + 1
    swapped, and a new addend stays only if no mut[i] meets the plain running sum."""
    alpha = [0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 3.5]

    def state(seq):
        pre = [0.0]
        for a in seq:
            pre.append(pre[-1] + a)
        mut = [fold(seq[i + 2:], (pre[i] + seq[i + 1]) + seq[i]) for i in range(1, len(seq) - 1)]
        return pre[-1], mut

    seq = [1.0]
    base, mut = 1.0, []
    guard = 0
    while len(seq) < L:
        guard += 1
        assert guard < 100 * L + 1000, "craft_sequence does not converge"
        prev = fold(seq[:-1])
        for c in rng.permutation(alpha).tolist():
            a = c * U
            nb = base + a
            nm = [v + a for v in mut] + ([(prev + a) + seq[-1]] if len(seq) >= 2 else [])
            if all(v != nb for v in nm):
                seq.append(a)
                base, mut = nb, nm
                break
        else:
            seq = seq[:-2] if len(seq) > 3 else [1.0]
            base, mut = state(seq)
    assert len(mut) == L - 2 and all(v != base for v in mut)
    return seq


def noisy(rng, count, lo=-3, hi=3):
    return np.ldexp(1.0 + rng.random(count), rng.integers(lo, hi, count).astype(np.int32))


def noisy_x(rng, n):
    x = np.ldexp(1.0 + rng.random(n), rng.integers(-10, 10, n).astype(np.int32))
    x[rng.random(n) < 0.04] = 0.0
    return x


class BuildCase:
    """name, flat (node_id, node_type, rowptr, dst, etype, w -- w is the first form's), forms {name: w}, x, seed, claims"""

    def __init__(self, name, flat, forms, x, seed, claims):
        self.name, self.flat, self.forms, self.x, self.seed, self.claims = name, flat, forms, x, seed, claims
        self.n, self.m = len(flat["rowptr"]) - 1, len(flat["dst"])
        self._norm, self._ref = {}, {}
        for a in list(flat.values()) + list(forms.values()) + [x]:
            a.setflags(write=False)

    def flat_of(self, form):
        return dict(self.flat, w=self.forms[form])

    def norm(self, form):
        if form not in self._norm:
            self._norm[form] = normalise(self.flat, self.forms[form])
        return self._norm[form]

    def reference(self, form):
        """computed once and shared: (norm, nextRank of one deliverRanks)"""
        if form not in self._ref:
            y = deliver_reference(self.flat, self.norm(form), self.x, self.seed)
            y.setflags(write=False)
            self._ref[form] = y
        return self.norm(form), self._ref[form]

    def item_ids(self):
        return [int(v) for v in self.flat["node_id"][self.flat["node_type"] == NODE_ITEM]]

    def plan(self, form):
        nm = self.norm(form)
        keep = self.flat["etype"] != EDGE_UNDEFINED
        deg = np.bincount(self.flat["dst"][keep], minlength=self.n) if keep.any() else np.zeros(self.n, dtype=np.int64)
        return sort_plan(self.n, self.m, nm["nnz"], int(deg.max(initial=0)), self.item_ids())


def default_types(n):
    t = np.full(n, NODE_USER, dtype=np.uint8)
    t[2::3] = NODE_ITEM                                            # ITEM and non-ITEM rows interleaved
    return t


def make_case(name, rng, general, lens, n=None, rows=(), undefined=(), undef_every=0, tmax=None, hub_ranges=False, hub_links=0,
              craft=True, dst=None, node_type=None, node_id=None, forms=("weighted", "uniform"), tweak=None, claims=None):
    """lens: the lengths of the leading rows (the rest are empty).  general: pad with dangling rows to ONE_LAUNCH_MAX_N + 1
    nodes unless n is given.  rows: source rows named for the row pass.  undefined: raw positions set UNDEFINED (and every
    undef_every-th link).  Links go to scattered targets below tmax, never to the hub (row tmax - 1), which takes one link from
    chosen single-link rows: one per 64-key step of the link sort's ranges (hub_ranges) or the first hub_links of them."""
    lens = np.asarray(lens, dtype=np.int64)
    n = max(len(lens), n or ((MAXN + 1) if general else 1))
    m = int(lens.sum())
    assert one_launch(n, m) != general, (name, n, m)
    rowptr = np.zeros(n + 1, dtype=np.int64)
    rowptr[1:len(lens) + 1] = np.cumsum(lens)
    rowptr[len(lens) + 1:] = m
    tmax = tmax or n
    hub = tmax - 1
    q = np.arange(m, dtype=np.int64)
    d_ = (q * 2654435761 + 12345) % max(1, tmax - 1) if dst is None else np.asarray(dst, dtype=np.int64)
    et = (1 + q % 7).astype(np.uint8)
    if undef_every:
        et[undef_every // 2::undef_every] = EDGE_UNDEFINED
    et[np.asarray(undefined, dtype=np.int64)] = EDGE_UNDEFINED
    x = noisy_x(rng, n)
    src = np.repeat(np.arange(n), np.diff(rowptr))
    # ---- the hub's in-list
    claims = dict(claims or {})
    ones = np.nonzero(lens == 1)[0]
    planted = []
    if hub_ranges or hub_links:
        ones = ones[ones != hub]
        pos1 = rowptr[ones]
        if hub_links:
            planted = ones[:hub_links].tolist()
        else:
            # one source in every 64-key step of every range (a wave's step of the one-workgroup sort; a wave's share of a
            # 256-key sub-tile of the multi-block scatter) and the last one of every range; past 70 000 links the ends of
            # every block only.  (Never two neighbouring rows: a link attributed to the row next door must bring another rank.)
            form = sort_form(one_launch(n, m), m, bit_length(n))
            ranges = [r for r in sort_ranges(form, m) if r[1] > r[0]]
            units = [(u, min(u + WAVE, b)) for a, b in ranges for u in range(a, b, WAVE)] if m <= 70000 else ranges
            first = np.searchsorted(pos1, [u[0] for u in units], side="left")
            last = np.searchsorted(pos1, [r[1] for r in ranges], side="left") - 1
            pick = {int(ones[k]) for k, u in zip(first.tolist(), units) if k < len(ones) and pos1[k] < u[1]}
            pick |= {int(ones[k]) for k, r in zip(last.tolist(), ranges) if k >= 0 and pos1[k] >= r[0]}
            for v in sorted(pick):
                if not planted or planted[-1] != v - 1:
                    planted.append(v)
            claims["hub_ranges"], claims["hub_units"] = ranges, units
        assert len(planted) == len(set(planted)) and (not hub_links or len(planted) == hub_links), name
        pp = rowptr[planted]
        d_[pp] = hub
        et[pp] = EDGE_FRIENDSHIP
        if craft and len(planted) >= 3:
            x[planted] = 2.0 * np.array(craft_sequence(rng, len(planted)))
            pset = set(planted)
            for u in planted:                                       # a neighbour's rank must not be the planted one's
                for v in (u - 1, u + 1):
                    if 0 <= v < n and v not in pset and (x[v] == x[u] or x[v] == 0.0):
                        x[v] = x[v] * 1.25 + 1.0
            claims["in_rows"] = [hub]
        claims["hub"], claims["planted"] = hub, planted
    # ---- weights
    w = noisy(rng, m)
    cu = 0.1 * (1 + np.arange(n) % 3)
    wu = cu[src].copy()
    wu[et == EDGE_UNDEFINED] = 7.0                                  # (an UNDEFINED link's weight never counts)
    fl = dict(node_id=(np.arange(n, dtype=np.int64) * 3 + 11) if node_id is None else np.asarray(node_id, dtype=np.int64),
              node_type=default_types(n) if node_type is None else np.asarray(node_type, dtype=np.uint8),
              rowptr=rowptr, dst=d_.astype(np.int32), etype=et, w=w)
    fm = {}
    if "weighted" in forms:
        fm["weighted"] = w
    if "uniform" in forms:
        fm["uniform"] = wu
    if tweak:
        tweak(fl, fm)
    seed = int(rng.integers(0, n))
    case = BuildCase(name, fl, fm, x, seed, dict(claims, rows=list(rows), general=general))
    if "weighted" in fm and rows:
        w = fm["weighted"].copy()
        for i in rows:
            b, e = int(rowptr[i]), int(rowptr[i + 1])
            for _ in range(400):
                if not row_survivors(case, i, w):
                    break
                w[b:e] = noisy(rng, e - b)
            else:
                raise AssertionError((name, i, "cannot be made sensitive"))
        case.forms["weighted"] = w
        w.setflags(write=False)
        case.flat["w"] = w
    return case


def spread_lens(m, max_rows):
    """row lengths 1, a, 1, b, ..., 1 (every other row a single link: the hub's sources) that add up to exactly m"""
    if m <= 2:
        return [1] * m
    avg = max(3, -(-m // max(1, int(0.45 * max_rows))))
    out, s, i = [], 0, 0
    while s < m:
        L = 1 if i % 2 == 0 else avg + (i % 5) - 2
        L = min(L, m - s)
        out.append(L)
        s += L
        i += 1
    if len(out) >= 3 and out[-1] == 1 and out[-2] == 1:
        out[-3:] = [out[-3] + 1, 1]
    elif out[-1] == 2 and len(out) > 1:                              # the very last link is a single-link row's: the last range's source
        out[-2:] = [2, 1]
    elif out[-1] > 1:
        out[-1] -= 1
        out.append(1)
    assert len(out) <= max_rows and sum(out) == m, (m, max_rows, len(out))
    return out


def _row_pass_cases(rng):
    out = []
    for general in (False, True):
        C = K_["RP_CAP"] if general else K_["BS_CAP"]
        tag = "general" if general else "one_launch"
        mk = lambda name, lens, **kw: out.append(make_case(f"{name}_{tag}", rng, general, lens, **kw))
        # a, b, c: rows ending at tile offsets CAP - 1, CAP and CAP + 1; row 2 starts exactly at the tile start; row 3 spans two tiles
        mk("rows_end_at_cap_minus_1_cap_cap_plus_1_then_span_two_tiles", [C - 1, 1, 1, C + 5, 3, 0, 9], rows=[3],
           claims=dict(ends={0: C - 1, 1: C, 2: C + 1}, starts_at_tile={2: 1}, spans={3: 2}))
        # d: a row over three tiles (and one over four) in a group of <= 8 CAP links
        mk("row_spans_three_and_four_tiles", [7, 2 * C + 9, 5, 3 * C + 2, 1, 4], rows=[1, 3], claims=dict(spans={1: 3, 3: 4}))
        # e: 4k, 4k + 1, 4k + 2, 4k + 3 entries of the crossing row before the edge (the 4-wide LDS loop and its scalar tail)
        lens, named, before = [], [], {}
        for r in range(4):
            lens += [C - (12 + r), 12 + r + 6] + [1] * 62
            named.append(64 * r + 1)
            before[64 * r + 1] = 12 + r
        mk("piece_of_4k_plus_0_1_2_3_before_the_edge", lens, rows=named, claims=dict(before_edge=before))
        # f: a group of exactly 8 CAP links (tiled) and of 8 CAP + 1 (long rows)
        base = 8 * C // 64
        per_tile = C // base
        mk("group_of_exactly_8_cap_links_is_tiled", [base + 5] + [base] * 62 + [base - 5], rows=[per_tile - 1, 3 * per_tile - 1, 7 * per_tile - 1],
           claims=dict(branch={0: "tiled"}, group_links={0: 8 * C}))
        mk("group_of_8_cap_plus_1_links_is_long", [base + 5] + [base] * 62 + [base - 4], rows=[0, per_tile - 1, 63],
           claims=dict(branch={0: "long"}, group_links={0: 8 * C + 1}))
        # g: long-row branch: rows of 8k - 1, 8k, 8k + 1 links, one link and none beside the rows that make the group long
        mk("long_branch_rows_of_8k_minus_1_8k_8k_plus_1_one_and_none", [39, 40, 41, 1, 0, 8 * C, 17] + [3] * 57, rows=[0, 1, 2, 5, 6],
           claims=dict(branch={0: "long"}, lens={0: 39, 1: 40, 2: 41, 3: 1, 4: 0}))
        # i: n % 64 in {0, 1, 63}; the last group's final link sits in a sweep-2 lane >= nrows where the group is short
        for rem in (0, 1, 63):
            n = ((MAXN + 64) if general else 128) + rem
            nrows = rem or 64
            first = n - nrows
            last = [C - 5, 11] + [1] * (nrows - 2) if nrows > 1 else [C + 70]
            last[-1 if nrows == 1 else 1] += (-sum(last)) % 64                     # the group's last link in lane 63
            mk(f"n_mod_64_is_{rem}_last_group_crosses_a_tile", [3, 0, 2] + [0] * (first - 3) + last, n=n, rows=[first + (0 if nrows == 1 else 1)],
               claims=dict(last_group_rows=nrows, last_link_lane=63))
        # j: a whole group of empty rows; empty rows on both sides of a tile-crossing row
        mk("empty_group_and_empty_rows_around_a_crossing_row", [0] * 64 + [C - 4, 0, 0, 12, 0, 0, 5, 0], rows=[67],
           claims=dict(empty_groups=[0], empty_neighbours={67: (65, 66, 68, 69)}))
        # k: UNDEFINED links: a row of nothing else; a first link UNDEFINED with a weight of its own; one on each side of an edge
        mk("undefined_only_row_first_link_and_both_sides_of_an_edge", [4, 6, C - 13, 9, 2, C - 5, 12],
           undefined=[0, 1, 2, 3, 4, C - 1, C, 2 * C - 1, 2 * C], rows=[3, 5],
           claims=dict(undefined_only_rows=[0], first_link_undefined=[1], undefined_at_edges=[C - 1, C, 2 * C - 1, 2 * C], patch_edges=[C, 2 * C]))
    # h: one-launch build, n > 512: wave 0 serves rows 512.. with the LDS arrays it used for rows 0..63
    C = K_["BS_CAP"]
    out.append(make_case("second_turn_of_a_wave_reuses_its_lds_one_launch", rng, False, [C - 3, 9] + [1] * 62 + [1] * 448 + [C - 2, 7] + [2] * 30,
                         n=600, rows=[1, 513], claims=dict(turns={1: (0, 0), 513: (0, 1)})))
    return out


def _flag_cases(rng):
    out = []
    for general in (False, True):
        C = K_["RP_CAP"] if general else K_["BS_CAP"]
        tag = "general" if general else "one_launch"
        lens = [C - 1, 1, 1, C + 5, 3, 2, 9]
        last = 2 * C + 5                                               # the last link of row 3, which crosses the edge at 2 CAP

        def nonuni(fl, fm):
            fm["uniform"][last] = fm["uniform"][last - 1] * 2
        out.append(make_case(f"only_nonuniform_weight_is_last_link_of_a_crossing_row_{tag}", rng, general, lens, forms=("uniform",), tweak=nonuni,
                             claims=dict(flags=dict(uniform=0, uniform_path=0), spans={3: 2})))

        def neg(fl, fm):
            fm["uniform"][C] = -2.0                                   # row 2: a single link
        out.append(make_case(f"one_negative_weight_{tag}", rng, general, lens, forms=("uniform",), tweak=neg,
                             claims=dict(flags=dict(uniform=1, uniform_path=0))))

        def inf(fl, fm):
            fm["uniform"][2 * C + 9:2 * C + 11] = 1e308                # row 5: two equal links whose sum overflows
        out.append(make_case(f"row_sum_overflows_to_inf_{tag}", rng, general, lens, forms=("uniform",), tweak=inf,
                             claims=dict(flags=dict(uniform=1, uniform_path=0), inf_rows=[5])))
    return out


def _sort_cases(rng):
    out = []
    # n: n on both sides of 2^8 and 2^16 with UNDEFINED links (sentinel key n); general n = 255 / 256 by more links than one launch takes
    for n, m, general in ((255, 3000, False), (256, 3000, False), (255, MAXM + 1, True), (256, MAXM + 1, True),
                          (65535, 30000, True), (65536, 30000, True)):
        out.append(make_case(f"link_sort_n_{n}_{'general' if general else 'one_launch'}", rng, general, spread_lens(m, n), n=n, undef_every=13,
                             hub_ranges=True, claims=dict(link_passes=(bit_length(n) + 7) // 8)))
    # o, p: the link count at the sort's form and range edges
    for m in (1, 63, 64, 1023, 1025, 20480, 20481, 65536):
        out.append(make_case(f"link_sort_m_{m}_one_launch", rng, False, spread_lens(m, 6000), n=6000, undef_every=17, hub_ranges=True,
                             claims=dict(link_form="body")))
    for m, form in ((1, "small"), (63, "small"), (64, "small"), (1023, "small"), (1025, "small"), (20480, "small"), (20481, "multi"),
                    (65536, "multi"), (65537, "multi"), (6 * SORT_CHUNK + 1, "multi")):
        out.append(make_case(f"link_sort_m_{m}_general", rng, True, spread_lens(m, MAXN + 1), undef_every=17, hub_ranges=True,
                             claims=dict(link_form=form, last_block_keys=(m - 1) % SORT_CHUNK + 1 if form == "multi" else None)))
    # r: all targets below 256 while n >= 256: the second pass of the link sort is the constant-digit copy
    for general in (False, True):
        out.append(make_case(f"all_targets_below_256_second_pass_is_a_copy_{'general' if general else 'one_launch'}", rng, general,
                             spread_lens(3000, 600), n=None if general else 600, tmax=256, hub_ranges=True, claims=dict(constant_digit_pass=1, link_passes=2)))
    return out


def _big_sort_case(rng):
    # q: 257 blocks: the second chunk of the scan's carry loop; the hub takes a link from every block
    m = 256 * SORT_CHUNK + 1
    return make_case(BIG_NAME, rng, True, spread_lens(m, 120000), n=120000, undef_every=19, hub_ranges=True,
                     claims=dict(link_form="multi", blocks=257))


def _order_cases(rng):
    out = []
    # t: one-launch build: the row order's key width follows the largest in-degree
    n = 600
    out.append(make_case("max_in_degree_0_one_launch", rng, False, [2, 0, 3], n=n, undefined=[0, 1, 2, 3, 4], claims=dict(max_in_deg=0)))
    out.append(make_case("max_in_degree_1_one_launch", rng, False, [1] * 300, n=n, dst=(np.arange(300) * 7 + 3) % n, claims=dict(max_in_deg=1)))
    for deg in (255, 256):
        # (the hub's sources are every other row, so that no two of them are neighbours and its in-list can be crafted)
        out.append(make_case(f"max_in_degree_{deg}_one_launch", rng, False, [1, 2] * deg, n=n, hub_links=deg, claims=dict(max_in_deg=deg)))
    # u: general build: the row orders' key width follows the explicit link count -- key_bits(nnz) for row_order (a pass more
    # from 256 and 65 536 on), one bit more for row_order_x (a pass more from 128 and 32 768 on)
    for nnz in (0, 127, 128, 255, 256, 32767, 32768, 65535, 65536):
        m = nnz + 3
        # (three UNDEFINED links inside rows of several links: none of them one of the hub's single-link sources)
        out.append(make_case(f"explicit_links_{nnz}_general", rng, True, spread_lens(m, MAXN + 1), undefined=[1, 2, 5] if nnz else [0, 1, 2],
                             hub_ranges=nnz > 0, claims=dict(nnz=nnz)))
    return out


def _item_cases(rng):
    """dangling seeds: every candidate ties at +0.0 and the ranked list IS the item order"""
    out = []
    for general in (False, True):
        tag = "general" if general else "one_launch"
        n = (MAXN + 1) if general else 300
        lens = [2, 1, 0, 3, 1]                                         # rows 0, 1, 3, 4 link; every other row is dangling
        dst = [5, 9, 5, 7, 9, 11, 2]
        user = lambda: np.full(n, NODE_USER, dtype=np.uint8)

        def mk(name, types, ids, lens=lens, dst=dst, n=n, **claims):
            nid = np.arange(n, dtype=np.int64) * 3 + 11
            it = np.nonzero(types == NODE_ITEM)[0]
            if ids is not None:
                nid[it] = ids
            seeds = [int(v) for v in np.nonzero(types != NODE_ITEM)[0] if v >= 10][:2]
            seeds += [int(v) for v in it if v >= 10][:max(1, 3 - len(seeds))]
            out.append(make_case(f"{name}_{tag}", rng, general, lens, n=n, dst=dst, node_type=types, node_id=nid,
                                 claims=dict(claims, item_seeds=seeds, n_items=len(it))))

        mk("no_items", user(), None)
        t = user(); t[40] = NODE_ITEM
        mk("one_item", t, None)
        if not general:
            mk("every_node_an_item", np.full(n, NODE_ITEM, dtype=np.uint8), None)
        else:
            # (the general build by more links than one launch takes: parallel links on four rows; top_n = n stays <= 1024)
            big = [20000, 20000, 20000, MAXM + 1 - 60000]
            mk("every_node_an_item", np.full(300, NODE_ITEM, dtype=np.uint8), None, lens=big, dst=(np.arange(MAXM + 1) * 2654435761 + 12345) % 300, n=300)
        t = user(); t[12:252:6] = NODE_ITEM                            # 40 items interleaved with the other types
        k = int((t == NODE_ITEM).sum())
        for span in (255, 256, 65535, 65536, 1 << 32):
            lo = -1000 - span // 2                                     # negative ids, the range straddles zero
            mid = rng.choice(np.arange(1, min(span, 1 << 16)), size=k - 2, replace=False).astype(np.int64) * (span // min(span, 1 << 16))
            ids = rng.permutation(np.concatenate([[0, span], mid]).astype(np.int64)) + lo      # both ends of the range, non-monotone
            mk(f"item_id_range_{span}", t, ids, id_span=span)
        ids = rng.permutation(np.concatenate([[I64_MIN, I64_MAX, -1, 0, 1], rng.integers(-(1 << 62), 1 << 62, k - 5)]).astype(np.int64))
        mk("item_ids_span_int64_min_to_max", t, ids, id_span=(1 << 64) - 1)
    return out


def make_cases():
    rng = np.random.default_rng(20241021)
    return _row_pass_cases(rng) + _flag_cases(rng) + _sort_cases(rng) + _order_cases(rng) + _item_cases(rng)


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = make_cases()
    return _CASES


def case_forms():
    return [(c, f) for c in cases() for f in c.forms]


BIG_NAME = "link_sort_m_1048577_is_257_blocks_general"
BIG_FORMS = ("weighted", "uniform")
_BIG = None


def big_case():
    """the 1 048 577-link case, built on first use: collecting the suite does not pay for it"""
    global _BIG
    if _BIG is None:
        _BIG = _big_sort_case(np.random.default_rng(20241022))
    return _BIG


def order_cases():
    """the cases that put the row orders' sorts on their pass-count edges (t, u; v: every one interleaves ITEM rows)"""
    return [c for c in cases() if "max_in_deg" in c.claims or "nnz" in c.claims]


# the row-pass cases whose tile edges the incremental rebuild patches (a to e and k)
PATCH_PREFIXES = ("rows_end_at_cap", "row_spans_three", "piece_of_4k", "undefined_only_row")


def patch_positions(case):
    """the raw links on each side of every tile edge that falls inside a named row"""
    f = case.flat
    pos = []
    for i in case.claims["rows"]:
        b = int(f["rowptr"][i])
        for k in row_edges(case.n, case.m, f["rowptr"], i):
            pos += [b + k - 1, b + k]
    return sorted(set(pos))
