"""The cases of tests/small_cases.py are what they claim to be -- shown from the oracle alone, so that a green run of
tests/test_gpu_small_edges.py means that small.hip's fold passes, its capacity edge and its long-row chunks were exercised."""
import numpy as np
import pytest

from tests import graphgen as gg
from tests import small_cases as sc
from tests.binade_scan_model import bits, chain_sum

STEPS = range(10)                   # the device tests run T <= 10: steps 1 .. 10 add the sequences of t = 0 .. 9
ALL = sorted({**sc.ONE_LAUNCH, **sc.TOO_LONG})


def ds_of(name):
    return {"Cadversarial": (0.5, sc.D15), "Cties": (0.5, sc.D15), "Csubnormal0": (0.0, sc.D15), "A1281": (sc.D15, 0.0, 1.0), "Dedges": (sc.D15, 0.0, 1.0)}.get(name, (sc.D15,))


@pytest.mark.parametrize("name", ALL)
def test_case_fits_and_has_the_named_length(name):
    g, seed, mlen = sc.case(name)
    n = len(g["node_id"])
    assert sc.fits_small_path(g)                                        # small_path_ok's limits, as numbers:
    assert n <= 6144 and int((g["node_type"] == gg.NODE_ITEM).sum()) <= 4096 and len(g["dst"]) <= 65536
    assert sc.mlen_of(g, seed) == mlen
    assert (mlen <= 12288) == (name in sc.ONE_LAUNCH)                   # small_path_seed_ok
    # the items that hear from the seed alone carry its value of the step before into the ranked list
    deg = sc.in_degrees(g)
    private = [v for v in np.flatnonzero((deg == 1) & (g["node_type"] == gg.NODE_ITEM)) if sc.in_links(g, v)[1][0] == seed]
    if name not in ("B12288quiet", "B12289quiet"):
        assert len(private) >= sc.N_PRIVATE
        liked = set(g["dst"][g["rowptr"][seed]:g["rowptr"][seed + 1]][g["etype"][g["rowptr"][seed]:g["rowptr"][seed + 1]] == gg.EDGE_LIKE].tolist())
        assert len([v for v in private if v not in liked]) >= sc.N_PRIVATE


@pytest.mark.parametrize("name", ALL)
def test_replay_equals_the_oracle(name):
    """seed_row_sequence, added in order, is the oracle's seed entry of the next step, bit for bit -- and so is the model of
    the binade scan over it."""
    g, seed, mlen = sc.case(name)
    F = sc.flat_graph(name)
    for d in ds_of(name):
        for t in STEPS:
            seq = sc.seed_row_sequence(F, seed, d, t)
            assert len(seq) == mlen
            x, _ = F.model_run(d, seed, 0, t + 1)
            assert bits(sc.replay(seq)) == bits(float(x[seed])), (d, t)
            if t in (1, 9):
                assert bits(chain_sum(seq.tolist(), block=sc.SM_R)[0]) == bits(float(x[seed])), (d, t)


def test_capacity_numbers():
    g0, _, _ = sc.case("B12288")
    g1, _, _ = sc.case("B12289")
    for g in (g0, g1):
        assert len(g["node_id"]) == 6144 == sc.SM_MAX_N
        assert int((g["node_type"] == gg.NODE_ITEM).sum()) == 4096 == sc.SM_MAX_ITEMS
        assert int((g["node_type"][:2048] == gg.NODE_USER).all())
    p, src = sc.in_links(g0, 0)
    assert len(np.unique(src)) == 6143 and len(p) == 6144 and 6144 + len(p) == 12288 == sc.SM_MCAP
    p, src = sc.in_links(g1, 0)
    assert len(np.unique(src)) == 6143 and len(p) == 6145 and 6144 + len(p) == 12289
    assert len(g1["dst"]) == len(g0["dst"]) + 1                         # one more multi-edge, nothing else
    assert sc.mlen_of(g0, sc.B_QUIET_SEED) == 6146


@pytest.mark.parametrize("mlen", sc.A_MLENS)
def test_length_edges_notice_their_last_addend(mlen):
    """The links into the seed carry distinct weights that are no powers of two, the last two places of the sequence (node
    n - 1's link and restart addends) are non-zero at step 2, and dropping or doubling the last one changes the seed's value."""
    assert mlen in (255, 256, 257, 1279, 1280, 1281, 2304, 2305)
    assert (mlen - sc.SM_SEQ) % sc.SM_PASS in (1023, 0, 1)              # the last slot of a pass, a full pass, one addend over
    g, seed, _ = sc.case(f"A{mlen}")
    F = sc.flat_graph(f"A{mlen}")
    p, src = sc.in_links(g, seed)
    wn = F.w_norm[p]
    assert len(np.unique(wn)) == len(wn) == mlen - len(g["node_id"])
    assert ((wn.view(np.uint64) & ((1 << 52) - 1)) != 0).all()
    seq = sc.seed_row_sequence(F, seed, sc.D15, 1)                      # the sequence step 2 adds
    assert seq[-1] > 0 and seq[-2] > 0 and src[-1] == len(g["node_id"]) - 1
    full = sc.replay(seq)
    x, _ = F.model_run(sc.D15, seed, 0, 2)
    assert bits(full) == bits(float(x[seed]))
    assert bits(sc.replay(seq[:-1])) != bits(full)
    assert bits(sc.replay(np.append(seq, seq[-1]))) != bits(full)
    assert bits(sc.replay(np.delete(seq, len(seq) - 2))) != bits(full)


def collect(name, d):
    F = sc.flat_graph(name)
    _, seed, _ = sc.case(name)
    return [sc.walk(sc.seed_row_sequence(F, seed, d, t)) for t in STEPS]


@pytest.mark.parametrize("d", [0.5, sc.D15])
def test_adversarial_hub_meets_its_counts(d):
    """Case C over steps 1 .. 10, at positions >= 256 only."""
    g, seed, _ = sc.case("Cadversarial")
    assert len(g["node_id"]) == 3000 and 3000 <= sc.in_degrees(g)[seed] == 4499 <= 6000
    ws = collect("Cadversarial", d)
    crossings = [q for w in ws for q in w["crossings"]]
    assert len(crossings) >= 20
    assert len(sc.off_first_lane(crossings)) >= 1
    assert sum(w["vanish"] for w in ws) >= 100
    assert all(w["zero_run"] >= 16 for w in ws)                         # at every step, not only the sparse first ones
    assert all(w["zero_lanes"] >= 1 for w in ws)                        # ... and a whole lane of a pass is zero
    assert sum(w["larger"] for w in ws) >= 1
    assert all(w["larger"] >= 1 for w in ws[1:])                        # the seed's restart addend, in the middle of a pass


def test_constructed_ties_meet_both_parities():
    """Random weights give no exact half-ulp addends, so they are constructed (c1 = 0.5, power-of-two weights, row sums that
    are powers of two): at steps 2 and 3 hundreds of addends are exactly half an ulp of the running sum, on either parity."""
    g, seed, _ = sc.case("Cties")
    assert len(g["node_id"]) == 4096 and 3000 <= sc.in_degrees(g)[seed] <= 6000
    assert collect("Cadversarial", 0.5)[1]["ties_even"] + collect("Cadversarial", 0.5)[1]["ties_odd"] == 0
    ws = collect("Cties", 0.5)
    for t in (1, 2):
        assert ws[t]["ties_even"] >= 10 and ws[t]["ties_odd"] >= 10, t
        assert ws[t]["vanish"] >= 100
    assert len(ws[1]["crossings"]) >= 1
    x, _ = sc.flat_graph("Cties").model_run(0.5, seed, 0, 1)
    assert x[seed] == 2048.0 and (x[1:2049] == 1.0).all()               # the construction's premise


def test_subnormal_start_of_the_passes():
    """The first pass receives a zero running sum at step 1 and a subnormal one at every later step (wave_fold_exact's
    eb == 0 branch), and the sum turns normal inside a pass."""
    ws = collect("Csubnormal", sc.D15)
    assert ws[0]["at_start"] == 0.0
    for t in STEPS[1:]:
        assert 0.0 < ws[t]["at_start"] < 2.0 ** -1022, t
        assert ws[t]["total"] > 1.0
    F = sc.flat_graph("Csubnormal")
    seq = sc.seed_row_sequence(F, sc.S_SEED, sc.D15, 1)
    first_normal = int(np.flatnonzero(seq >= 2.0 ** -1022)[0])
    assert first_normal >= sc.SM_SEQ + sc.SM_PASS and (first_normal - sc.SM_SEQ) % sc.SM_PASS >= sc.SM_R
    assert 0.0 < sc.replay(seq[:first_normal]) < 2.0 ** -1022


def test_closed_subnormal_sum_counts_every_addend():
    """Csubnormal0 at d = 0: nothing but the first-hop users feeds the seed, so step 2's sum starts subnormal when the passes
    begin, turns normal inside the first pass behind its first lane, and ends in the lowest binades -- where dropping any one
    addend of the pass's first lane changes its bits.  Step 3 carries it to the items that hear from the seed alone."""
    g, seed, _ = sc.case("Csubnormal0")
    F = sc.flat_graph("Csubnormal0")
    assert F.dangling[800:].sum() == 0 and (sc.in_links(g, seed)[1] < seed).all()
    seq = sc.seed_row_sequence(F, seed, 0.0, 1)
    w = sc.walk(seq)
    assert 0.0 < w["at_start"] < 2.0 ** -1022 <= w["total"] < 2.0 ** -1000
    s, turn = 0.0, None
    for q, a in enumerate(seq.tolist()):
        s += a
        if turn is None and s >= 2.0 ** -1022:
            turn = q
    assert sc.SM_SEQ + sc.SM_R <= turn < sc.SM_SEQ + sc.SM_PASS
    lane0 = [q for q in range(sc.SM_SEQ, sc.SM_SEQ + sc.SM_R) if seq[q] != 0.0]
    assert len(lane0) >= 4
    assert all(bits(sc.replay(np.delete(seq, q))) != bits(w["total"]) for q in lane0)
    x3, _ = F.model_run(0.0, seed, 0, 3)
    assert (x3[800:800 + sc.N_PRIVATE] > 0).all()


@pytest.mark.parametrize("name", sorted(sc.D_LONG_ROWS))
def test_long_rows_are_dialled_and_order_dependent(name):
    g, seed, _ = sc.case(name)
    F = sc.flat_graph(name)
    deg = sc.in_degrees(g)
    kind = name[1:]
    targets = sc.rows_targets(kind)
    for j, ln in targets.items():
        assert deg[j] == ln and j != seed
        assert len(np.unique(F.w_norm[sc.in_links(g, j)[0]])) > 1 or ln <= 1
    assert int((deg >= sc.LONG_ROW).sum()) == sc.D_LONG_ROWS[name]      # small.hip's n_long
    if name == "Dedges":
        assert sorted(targets.values())[-9:] == [127, 128, 129, 191, 192, 193, 255, 256, 257]
    if name == "Dmany":
        assert sc.D_LONG_ROWS[name] == 20 > sc.SM_WAVES - 1
    if name == "Dseedlong":
        assert deg[seed] == 170 >= sc.LONG_ROW and sc.D_LONG_ROWS[name] > sc.SM_WAVES - 1
        assert 0 < int((deg > deg[seed]).sum()) < sc.D_LONG_ROWS[name] - 1      # the seed sits inside the long rows' order
    if name == "Dseed0":
        assert deg[seed] == 0
    # the short-row walk's remainders: rows of 0, 1, 3, 4, 5, 7 and 8 in-links, reached by T = 2
    x2, _ = F.model_run(sc.D15, seed, 0, 2)
    for k in (0, 1, 3, 4, 5, 7, 8):
        rows = [j for j, ln in targets.items() if ln == k]
        assert rows and all((x2[j] > 0) == (k > 0) for j in rows), k
    # every row of >= 127 in-links: at some step the reversed order gives other bits
    for j, ln in targets.items():
        if ln < 127:
            continue
        assert any(bits(sc.replay(s)) != bits(sc.replay(s[::-1]))
                   for s in (sc.row_sequence(F, j, sc.D15, seed, t) for t in STEPS)), j
        s = sc.row_sequence(F, j, sc.D15, seed, 1)
        x, _ = F.model_run(sc.D15, seed, 0, 2)
        assert len(s) == ln and bits(sc.replay(s)) == bits(float(x[j]))


def test_seed_as_a_long_row_is_order_dependent_too():
    F = sc.flat_graph("Dseedlong")
    assert any(bits(sc.replay(s)) != bits(sc.replay(s[::-1])) for s in (sc.seed_row_sequence(F, 0, sc.D15, t) for t in STEPS))
