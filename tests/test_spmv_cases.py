"""The cases of tests/spmv_cases.py proved on the CPU, before tests/test_gpu_spmv_edges.py hands them to the kernels.

This file holds a small model of what the device decides for a graph -- the in-degree orders and the bin split of
launch_spmv_exact, the hub kernel's prefix and pass counts, sweep_prepare's take / K / ITEM-rows-only decision for a given
number of workgroups and the layout it builds (slots dealt s % nwg, per-(slot, block) word counts, per-wave streams, visited
blocks) -- and proves for every case: its claims hold in the model under the ascending AND the descending order of rows of
equal in-degree; the vectorised reference equals the plain loop (and chain_cases.deliver_reference on the small cases);
every row a case names as a target changes bits when its in-list is summed back to front; the constants the cases stand on
are the ones in the sources.  CPU only."""
import os
import re

import numpy as np
import pytest

from tests import chain_cases as cc
from tests import spmv_cases as sc

CASES = sc.cases()
IDS = [c.name for c in CASES]
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "recommendersystems_amd", "csrc")
K_ = sc.EXPECTED_CONSTANTS
WAVE, WPG, MAXK, GR, G = K_["WAVE"], K_["WPG"], K_["SW_MAXK"], K_["SW_GR"], K_["SW_G"]
TIES = ("ascending", "descending")
NCU_ASSUMED = (256, 304, 64)          # in-process sweep cases: the claims must hold whatever the CU count decides


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------------------- the model

def by_degree(rows, deg, tie):
    """rows by in-degree descending; equal degrees by index ascending or descending"""
    rows = np.asarray(rows, dtype=np.int64)
    idx = rows if tie == "ascending" else -rows
    return rows[np.lexsort((idx, -deg[rows]))]


def phase_orders(case, tie, two_phase):
    """row_order (one phase) or row_order_x (ITEM rows, then the others)"""
    deg = case.in_deg
    if not two_phase:
        return [by_degree(np.arange(case.n), deg, tie)]
    item = case.node_type == sc.NODE_ITEM
    return [by_degree(np.nonzero(item)[0], deg, tie), by_degree(np.nonzero(~item)[0], deg, tie)]


def bin_split(order, deg, hub_t):
    """launch_spmv_exact's `launch` on one order: the rows of the hub kernel and of the four bodies"""
    d = deg[order]
    nh, b0, b1, b2 = int((d >= hub_t).sum()), int((d >= K_["BIN_WAVE"]).sum()), int((d >= K_["BIN_16"]).sum()), int((d >= K_["BIN_4"]).sum())
    return {"hub": order[:nh], "wave": order[nh:b0], "g16": order[b0:b1], "g4": order[b1:b2], "lane": order[b2:]}


def waves_of(rows, body):
    rpw = {"wave": 1, "g16": WAVE // 16, "g4": WAVE // 4, "lane": WAVE}[body]
    return [rows[q:q + rpw] for q in range(0, len(rows), rpw)]


def sweep_decide(case, knobs, ncu, weighted):
    """sweep_prepare's decision: None, or {k, blocks, wgs, partial, order (the rows in sweep order, per tie)}"""
    hub_t, BN, min_n, wgs, _ = sc.knob_values(knobs)
    n, deg = case.n, case.in_deg
    if weighted or n < min_n or deg.sum() <= 0:
        return None
    item = case.node_type == sc.NODE_ITEM
    hub = deg >= hub_t
    a0, a1 = int((item & ~hub).sum()), int((~item & ~hub).sum())
    B = -(-n // BN)
    if B > 512 or hub_t > GR * 65535:
        return None
    nwg = wgs if wgs else ((ncu * 5) // 8 if hub.any() else ncu)
    nwg = max(1, min(nwg, ncu))
    slots_of = lambda r: -(-r // WAVE)
    n_sw, partial = a0 + a1, 0
    if -(-slots_of(n_sw) // (nwg * WPG)) > MAXK:
        need = -(-slots_of(a0) // (WPG * MAXK))
        if a0 <= 0 or a1 <= 0 or need > ncu:
            return None
        partial, n_sw, nwg = 1, a0, max(nwg, need)
    if n_sw <= 0:
        return None
    K = -(-slots_of(n_sw) // (nwg * WPG))
    if K > MAXK:
        return None
    return dict(k=K, blocks=B, wgs=nwg, partial=partial, n_sw=n_sw, BN=BN, hub_t=hub_t)


def sweep_layout(case, dec, tie):
    """the tables sweep_prepare builds for a decision: sweep order, per-row piece entries, per-(slot, block) word counts,
    per-workgroup visited blocks, per-wave piece lists (in stream order) and stream lengths"""
    deg, B, BN, nwg, K = case.in_deg, dec["blocks"], dec["BN"], dec["wgs"], dec["k"]
    ph = phase_orders(case, tie, True)
    order = np.concatenate([p[deg[p] < dec["hub_t"]] for p in (ph[:1] if dec["partial"] else ph)])
    assert len(order) == dec["n_sw"]
    ns = -(-len(order) // WAVE)
    ent = np.zeros((ns * WAVE, B), dtype=np.int64)
    for q, j in enumerate(order.tolist()):
        if j in case.rows:
            ent[q] = np.bincount(case.rows[j] // BN, minlength=B)
    words = -(-ent // GR)
    per_slot = words.reshape(ns, WAVE, B)
    scnt = per_slot.max(axis=1)
    exists = (np.arange(ns * WAVE) < len(order)).reshape(ns, WAVE)
    row_padding = any((per_slot[s][exists[s]].min(axis=0) < scnt[s]).any() for s in range(ns))
    visited, streams = [], {}
    for wg in range(nwg):
        mine = [s for s in range(wg, ns, nwg) if s // nwg < K * WPG]
        vis = [b for b in range(B) if any(scnt[s, b] for s in mine)]
        visited.append(vis)
        for wave in range(WPG):
            sl = [(i * WPG + wave) * nwg + wg for i in range(K)]
            pieces = [(int(scnt[s, b]) if s < ns else 0, s < ns) for b in vis for s in sl]
            streams[(wg, wave)] = pieces
            assert sum(c for c, _ in pieces) == sum(int(scnt[s].sum()) for s in sl if s < ns)
    refills = sum(len(v) for v in visited)
    if dec["partial"] and refills > 16 * nwg:
        return None
    return dict(order=order, ent=ent[:len(order)], scnt=scnt, visited=visited, streams=streams, row_padding=row_padding, ns=ns)


def sweep_features(case, dec, lay):
    f = set()
    n, BN, B = case.n, dec["BN"], dec["blocks"]
    r = n - (B - 1) * BN
    f.add(f"last_block_elems:{r}")
    if n % 2 == 1 and r == 1:
        f.add("last_pair_prev_block")
    if dec["n_sw"] % WAVE:
        f.add("n_sw_not_mult_64")
    if case.seed in lay["order"].tolist():
        f.add("seed_in_sweep")
    if lay["scnt"].max(initial=0) >= 40:
        f.add("piece_ge_40")
    if lay["row_padding"]:
        f.add("row_padding")
    for e in np.unique(lay["ent"]).tolist():
        f.add(f"word_padding:{e}")
    for vis in lay["visited"]:
        if not vis:
            f.add("wg_no_entries")
        if vis and vis[-1] - vis[0] + 1 != len(vis):
            f.add("wg_skips_block")
    for pieces in lay["streams"].values():
        T = sum(c for c, _ in pieces)
        f.add(f"T:{T}")
        pos, ones = 0, []
        for q, (c, real) in enumerate(pieces):
            end = pos + c
            if c >= G and end % G == 0:
                f.add("end_on_group")
            if c >= G + 1 and end % G == 1:
                f.add("end_after_group")
            if c >= G - 1 and end % G == G - 1:
                f.add("end_before_group")
            if c == 0 and real:
                f.add("empty_piece_visited")
                if q + 1 < len(pieces) and pieces[q + 1][0] == 0 and pieces[q + 1][1]:
                    f.add("two_empty_in_row")
                if q == len(pieces) - 1 and T > 0:
                    f.add("empty_last")
            if c == 1:
                ones.append(pos)
                if len(ones) >= 3 and ones[-3] + 2 == pos and ones[-3] // G == pos // G:
                    f.add("three_pieces_in_group")
            elif c > 1:
                ones = []
            pos = end
    return f


def step_model(case, knobs, weighted, tie, ncu=256):
    """what ONE dense step launches: {sweep: decision or None, hub_launches, binned_launches, splits: the bin splits}"""
    hub_t, _, _, _, two_phase = sc.knob_values(knobs)
    deg = case.in_deg
    dec = sweep_decide(case, knobs, ncu, weighted)
    lay = sweep_layout(case, dec, tie) if dec else None
    if dec and lay is None:
        dec = None
    splits = []
    if dec:
        ph = phase_orders(case, tie, True)
        hubs = [int((deg[p] >= hub_t).sum()) for p in ph]
        hub_launches = sum(h > 0 for h in hubs)
        if dec["partial"]:
            splits.append(bin_split(ph[1], deg, hub_t))
        binned = sum(1 for s in splits if sum(len(s[b]) for b in ("wave", "g16", "g4", "lane")) > 0)
    else:
        splits = [bin_split(p, deg, hub_t) for p in phase_orders(case, tie, two_phase) if len(p)]
        hub_launches = sum(len(s["hub"]) > 0 for s in splits)
        binned = sum(1 for s in splits if sum(len(s[b]) for b in ("wave", "g16", "g4", "lane")) > 0)
    return dict(sweep=dec, layout=lay, hub_launches=hub_launches, binned_launches=binned, splits=splits)


# ------------------------------------------------------------------------------------------------------------- the proofs

def test_case_names_are_unique_and_every_knob_set_has_cases():
    assert len(set(IDS)) == len(IDS)
    for knobs in sc.KNOBS:
        assert sc.cases_for(knobs), knobs
    for c in CASES:
        assert set(c.knobs) <= set(sc.KNOBS) and c.claims["targets"] and c.claims["branch"], c.name
        assert c.seed not in c.claims["targets"], c.name


@pytest.fixture(scope="module")
def refs():
    memo = {}

    def get(case, weighted):
        if (case.name, weighted) not in memo:
            r = sc.reference(case, weighted)
            r.setflags(write=False)
            memo[(case.name, weighted)] = r
        return memo[(case.name, weighted)]
    return get


@pytest.mark.parametrize("weighted", [False, True], ids=["valuefree", "weighted"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_references_agree_and_targets_depend_on_the_list_order(case, weighted, refs):
    ref = refs(case, weighted)
    loop = sc.loop_reference(case, weighted)
    assert (bits(ref) == bits(loop)).all(), case.name
    flat = case.flat(weighted)
    if len(flat["dst"]) <= 30000:                                   # the chain cases' own reference, link by link
        wn, dang = sc.normalised_fast(flat)
        wn2, dang2 = cc.normalised(flat)
        assert (bits(wn) == bits(wn2)).all() and (dang == dang2).all()
        assert (bits(ref) == bits(cc.deliver_reference(case, weighted))).all(), case.name
    # the weighted form: weights that differ inside a forward row (so a weight read at the wrong offset shows), same in-lists
    per_row = np.maximum.reduceat(flat["w"], flat["rowptr"][:-1][np.diff(flat["rowptr"]) > 0])
    assert (per_row.max() > 1.0) == weighted and (flat["w"].min() == 1.0)
    targets = case.claims["targets"]
    back = sc.loop_reference(case, weighted, reverse_rows=set(targets))
    same = [j for j in targets if bits(back)[j] == bits(ref)[j]]
    assert not same, (case.name, "rows whose sum does not depend on the order of the adds", same[:5])
    untouched = np.ones(case.n, dtype=bool)
    untouched[targets] = False
    assert (bits(back)[untouched] == bits(ref)[untouched]).all()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_claims_hold_in_the_model_under_both_tie_orders(case):
    cl = case.claims
    for knobs in case.knobs:
        hub_t = sc.knob_values(knobs)[0]
        in_process = knobs == "default"
        for tie in TIES:
            for weighted in (False, True):
                for ncu in (NCU_ASSUMED if in_process and cl["kernel"] == "sweep" else (256,)):
                    m = step_model(case, knobs, weighted, tie, ncu)
                    tag = (case.name, knobs, tie, weighted, ncu)
                    assert (m["sweep"] is not None) == (cl["kernel"] == "sweep" and not weighted), tag
                    assert m["hub_launches"] == cl["hub_launches"][1 if weighted else 0], (tag, m["hub_launches"])
                    if m["sweep"] is None:
                        assert m["binned_launches"] >= 1, tag
                    elif "binned_beside" in cl:
                        assert m["binned_launches"] == 1 and m["sweep"]["partial"] == 1, tag
                    if m["sweep"] is not None:
                        got = sweep_features(case, m["sweep"], m["layout"])
                        missing = [f for f in cl.get("features", []) if f not in got]
                        assert not missing, (tag, missing, sorted(got))
                        if "geometry" in cl:
                            assert {k: m["sweep"][k] for k in ("k", "blocks", "wgs", "partial")} == cl["geometry"], (tag, m["sweep"])
                        if "T" in cl:
                            Ts = sorted((sum(c for c, _ in p) for p in m["layout"]["streams"].values()), reverse=True)
                            assert Ts == sorted(cl["T"], reverse=True), (tag, Ts)
                    split = m["splits"][0] if m["splits"] else None
                    if "bins" in cl and not sc.knob_values(knobs)[4] and m["sweep"] is None:
                        assert {b: len(split[b]) for b in split} == cl["bins"], (tag, {b: len(split[b]) for b in split})
                    if m["sweep"] is None:
                        for s in m["splits"]:
                            for body in cl.get("partial_wave", []):
                                rpw = len(waves_of(np.arange(WAVE), body)[0])
                                if not sc.knob_values(knobs)[4]:
                                    assert len(s[body]) % rpw != 0, (tag, body)
                            for body in cl.get("mixed_wave", []):
                                d = case.in_deg[s[body]]
                                assert any({d.min(), d.max()} <= set(case.in_deg[w].tolist()) for w in waves_of(s[body], body)) and d.min() < d.max(), (tag, body)
                        if "seed_body" in cl:
                            assert any(case.seed in s[cl["seed_body"]].tolist() for s in m["splits"]), tag
        for L, want in cl.get("hub_rows", {}).items():
            assert L >= hub_t and (case.in_deg == L).any() and sc.hub_passes(L) == want, (case.name, L, sc.hub_passes(L))
        if "hub_types" in cl:
            hubs = case.in_deg >= hub_t
            assert sorted(set(case.node_type[hubs].tolist())) == sorted(cl["hub_types"]), case.name
    if cl.get("reads_last") is True:
        assert any(len(s) and s[-1] == case.n - 1 for j, s in case.rows.items() if j != case.seed), case.name
    elif cl.get("reads_last"):
        for j in cl["reads_last"]:
            assert j == case.seed or {case.n - 3, case.n - 2, case.n - 1} <= set(case.rows[j].tolist()), (case.name, j)


def test_the_case_set_covers_the_edges_the_kernels_decide_on():
    p = sc.PREFIX
    degs = {k: set() for k in sc.KNOBS}
    for c in CASES:
        for k in c.knobs:
            degs[k] |= set(np.unique(c.in_deg).tolist())
    assert set(sc.DEG_ALL) <= degs["default"] and set(sc.DEG_ALL) <= degs["phases"]
    assert {2047, 2048, 2049, p + 1536, p + 1537, p + 2047} <= degs["default"]
    assert {128, 255, 256, 257, p + 511, p + 512, p + 513, p + 1024, p + 1025, p + 1536, p + 1537, p + 2055} <= degs["hub128"]
    ns = {c.n for c in sc.cases_for("default") if c.claims["kernel"] == "sweep"}
    bn = sc.BN_DEFAULT
    assert ns == {65535, 65536, 65537, 65538, 4 * bn + 127, 4 * bn + 128, 4 * bn + 129}
    child = [c for k in ("sweep_w1", "sweep_w3") for c in sc.cases_for(k)]
    geo = {(c.claims["geometry"]["k"], c.claims["geometry"]["partial"]) for c in child}
    assert {(1, 0), (2, 0), (3, 0), (4, 0)} <= geo and any(p_ for _, p_ in geo)
    feats = set().union(*(c.claims.get("features", []) for c in child))
    want = {f"T:{t}" for t in (0, 1, 3, 4, 5, 15, 16, 17, 31, 32, 33)} | {f"last_block_elems:{r}" for r in (1, 2, 3, 127, 128)} | \
        {f"word_padding:{e}" for e in (1, 2, 3, 4, 5)} | {"end_on_group", "end_after_group", "end_before_group", "three_pieces_in_group",
                                                          "row_padding", "empty_piece_visited", "two_empty_in_row", "empty_last",
                                                          "wg_skips_block", "wg_no_entries", "n_sw_not_mult_64", "seed_in_sweep",
                                                          "last_pair_prev_block"}
    assert want <= feats | {f for c in sc.cases_for("default") for f in c.claims.get("features", [])}, sorted(want - feats)
    assert any("piece_ge_40" in c.claims.get("features", []) for c in sc.cases_for("default"))
    seed_bodies = {c.claims.get("seed_body") for c in CASES}
    assert {"lane", "g4", "g16", "wave", "hub"} <= seed_bodies
    assert any(int((c.in_deg >= 128).sum()) > K_["HUB_GRID"] for c in sc.cases_for("hub128"))


def test_the_levelled_hub_row_holds_the_pattern_it_claims():
    case = [c for c in CASES if "exact_addends" in c.claims][0]
    hub = case.claims["exact_addends"]
    for weighted in (False, True):
        a_in, in_ptr, _, _ = sc._parts(case, weighted)
        a = a_in[in_ptr[hub]:in_ptr[hub + 1]].tolist()
        assert (np.array(a) == 0.5 * case.x[case.rows[hub]]).all()
        s = cc.fold(a[:201])
        assert cc._mant(s) == 3 << 51 and 200 < sc.PREFIX                     # 1.5 * 2^E inside the one-by-one prefix
        u = 2.0 ** (cc._exp(s) - 1023 - 52)
        tail = np.array(a[201:])
        assert (tail == 0).any() and (tail == 0.5 * u).any() and ((tail > 0) & (tail < 2.3e-308)).any()


def test_odd_n_sweep_cases_fail_on_a_last_element_clamped_to_n_minus_3():
    """Sensitivity, by reasoning from the reference: before the odd-n patch in sweep.hip's SW_ENTER_BLOCK the 16-byte LDS
    refill clamped the last element of an odd-length z to its last whole pair's neighbour, so the LDS slot of z[n - 1] held
    z[n - 3].  Every value-free sweep case with odd n has rows (other than the seed's) that read z[n - 1], z[n - 1] differs
    from z[n - 3], and each such row's list-order sum changes bits with that substitution: those cases fail without the patch."""
    odd = [c for c in CASES if c.claims["kernel"] == "sweep" and c.n % 2 == 1]
    assert {65535, 65537, 4 * sc.BN_DEFAULT + 127, 4 * sc.BN_DEFAULT + 129, 385} <= {c.n for c in odd}
    for case in odd:
        n = case.n
        a_in, in_ptr, src_in, _ = sc._parts(case, False)
        flat = case.flat(False)
        z = lambda u: (1 - case.d) * case.x[u] * (1.0 / float(flat["rowptr"][u + 1] - flat["rowptr"][u]))
        assert z(n - 1) != z(n - 3) and (a_in[src_in == n - 1] == z(n - 1)).all()
        clamped = np.where(src_in == n - 1, z(n - 3), a_in).tolist()
        a = a_in.tolist()
        readers = [j for j, s in case.rows.items() if j != case.seed and s[-1] == n - 1 and case.in_deg[j] < sc.knob_values(case.knobs[0])[0]]
        assert readers, case.name
        changed = [j for j in readers if cc.fold(a[in_ptr[j]:in_ptr[j + 1]]) != cc.fold(clamped[in_ptr[j]:in_ptr[j + 1]])]
        assert len(changed) >= max(1, len(readers) // 2), (case.name, len(changed), len(readers))


def test_stats_mirrors_carry_the_spmv_counters_in_the_header_order():
    """rwr_stats in include/rwr.h, its ctypes mirror and the C# shim's RwrStats: same field names in the same order, the SpMV
    counters at the end (the struct grows at the end only), natural alignment giving the same offsets."""
    import ctypes as C
    from recommendersystems_amd import _lib as L
    root = os.path.dirname(CSRC.rstrip(os.sep))
    root = os.path.dirname(root)
    hdr = open(os.path.join(root, "include", "rwr.h")).read()
    body = re.search(r"typedef struct rwr_stats\s*\{(.*?)\}\s*rwr_stats;", hdr, re.S).group(1)
    fields = re.findall(r"\b(int32_t|int64_t|double)\s+(\w+)\s*;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}
    assert [(nm, ctype[t]) for t, nm in fields] == list(L.rwr_stats._fields_)
    tail = ["spmv_sweep_launches", "spmv_hub_launches", "spmv_binned_launches", "sweep_k", "sweep_blocks", "sweep_wgs", "sweep_partial"]
    assert [nm for _, nm in fields][-7:] == tail
    assert L.rwr_stats.spmv_sweep_launches.offset == L.rwr_stats.entry_live_launches.offset + 8
    assert C.sizeof(L.rwr_stats) == L.rwr_stats.sweep_partial.offset + 4 and C.sizeof(L.rwr_stats) % 8 == 0
    cs = open(os.path.join(root, "csharp", "Recommenders", "RWRBased", "Types.cs")).read()
    cs_body = re.search(r"struct RwrStats\s*\{(.*?)\}", cs, re.S).group(1)
    cs_fields, off = [], 0
    for typ, names in re.findall(r"public\s+(int|long|double)\s+([^;]+);", cs_body):
        size = {"int": 4, "long": 8, "double": 8}[typ]
        for name in [x.strip() for x in names.split(",")]:
            off = (off + size - 1) // size * size
            cs_fields.append((name, off, size))
            off += size
    assert cs_fields == [(nm, getattr(L.rwr_stats, nm).offset, getattr(L.rwr_stats, nm).size) for nm, _ in L.rwr_stats._fields_]
    native = open(os.path.join(root, "csharp", "Recommenders", "RWRBased", "Native.cs")).read()
    assert re.search(r"static extern int rwr_get_stats\(GraphHandle \w+, ref RwrStats \w+\)", native)
    hpp = open(os.path.join(root, "include", "recommenders", "rwr_based.hpp")).read()
    assert "rwr_stats stats() const" in hpp and "st.struct_size = (int32_t)sizeof(st);" in hpp


# ---- the constants the cases stand on, read out of the sources

def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _one(pattern, src):
    found = re.findall(pattern, src)
    assert len(found) == 1, (pattern, found)
    return int(found[0])


def read_constant(name):
    spmv, sweep, build, common = _src("spmv.hip"), _src("sweep.hip"), _src("build.hip"), _src("common.h")
    if name in ("SW_GR", "SW_G", "SW_D", "SW_MAXK"):
        return _one(r"constexpr int " + name + r" = (\d+);", sweep)
    if name == "WPG":
        return _one(r"const int wpg = (\d+);", sweep)
    if name == "BN_MAX":
        assert _one(r'getenv\("RWR_SWEEP_BN"\); return e \? atoi\(e\) : (\d+);', sweep) == _one(r"if \(BN > (\d+)\) BN = \d+;", sweep)
        return _one(r"if \(BN > \d+\) BN = (\d+);", sweep)
    if name == "BN_STEP":
        assert "BN &= ~127;" in sweep and _one(r"if \(BN < (\d+)\) BN = \d+;", sweep) == 128
        return 128
    if name == "SWEEP_MIN_N":
        return _one(r'getenv\("RWR_SWEEP_MIN_N"\); return e \? atol\(e\) : (\d+)l;', sweep)
    if name == "HUB_T":
        return _one(r'getenv\("RWR_HUB_T"\); return e \? atoi\(e\) : (\d+);', build)
    if name == "HUB_T_MIN":
        return _one(r"g->hub_t = hub_t_env < (\d+) \? \d+ : hub_t_env;", build)
    if name == "HS_R":
        assert "constexpr int HS_PASS = WAVE * HS_R;" in spmv
        return _one(r"constexpr int HS_R = (\d+);", spmv)
    if name == "HUB_PREFIX":
        return _one(r'RWR_TUNE_ENV\("RWR_HUB_PREFIX"\); return e \? atoi\(e\) : (\d+);', spmv)
    if name == "HUB_GRID":
        return _one(r"const unsigned grid = \(unsigned\)\(nh < (\d+) \? nh : \d+\);", spmv)
    if name in ("BIN_WAVE", "BIN_16", "BIN_4"):
        idx = {"BIN_WAVE": 0, "BIN_16": 1, "BIN_4": 2}[name]
        a = _one(r"g->bin_end\[%d\] \+= deg >= (\d+);" % idx, build)
        assert a == _one(r"g->x_bins\[ph\]\[%d\] \+= deg >= (\d+);" % idx, build)
        return a
    if name == "WAVE":
        return _one(r"constexpr int WAVE = (\d+);", common)
    raise KeyError(name)


@pytest.mark.parametrize("name", sorted(sc.EXPECTED_CONSTANTS))
def test_spmv_constant_is_where_the_cases_expect_it(name):
    got = read_constant(name)
    assert got == sc.EXPECTED_CONSTANTS[name], (
        f"{name} is {got} in the sources, but tests/spmv_cases.py builds its boundary cases around "
        f"{sc.EXPECTED_CONSTANTS[name]}: move those cases onto the new boundary, then update EXPECTED_CONSTANTS there")


def test_the_shipped_library_reads_the_group_and_prefix_knobs_in_the_experiments_build_only():
    """the lane body therefore only ever serves rows of <= 3 in-links (its 8-wide loop and its tails of 4 to 7 entries are
    not reachable in the shipped library), and the hub prefix is always 256"""
    spmv = _src("spmv.hip")
    assert 'RWR_TUNE_ENV("RWR_GROUP_ROWS"); return e ? atoi(e) : 2;' in spmv and 'RWR_TUNE_ENV("RWR_ROW_ORDER")' in spmv
    assert re.search(r"define RWR_TUNE_ENV\(\w+\) \(?\(?const char \*\)?\s*nullptr", _src("common.h") + _src("engine.h")) or \
        "RWR_EXPERIMENTS" in (_src("common.h") + _src("engine.h"))
