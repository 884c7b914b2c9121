"""The row-partitioned step, slab by slab and bit by bit: rwr_part_begin / rwr_part_local_step / rwr_part_finish_step /
rwr_part_step / rwr_part_rank on logical ranks (one HipSlabBackend per slab, one process), against tests/slab_double.py's
slab_partial -- an in-order numpy accumulation that test_slab_reference.py pins to a plain Python loop.

A rank's link-only partial y = (1-d) P_slab^T x is a per-row list-order sum from 0.0 (mulsd / addsd, no FMA): bitwise
predictable for any x, whatever the step counter makes of the step (marking, probing, dense).  Only the restart mass r (a
tree sum) and the cross-rank sum re-associate; r has a derived bound (restart_depth), the end-to-end check keeps the project's
1e-9.  No other tolerance.

Which code runs where, from partition.hip (vf = uniform slab graph; frontier = vf && G >= 8 && rows > 0 && part_steps < 4;
mark = frontier && part_steps < 2) and iterate.hip's launch_spmm_g (G == 1: launch_spmv_exact; G = 2, 4: k_spmm; G >= 8:
k_spmm_chunked):
  * value-free with lo > 0 (the shifted base Z0.p - lo * G, k_make_z / k_make_z_nz on a slab): every VF case but "whole";
    64-aligned and unaligned lo, a slab inside one bitmap word, the hub's single row: layouts lo_64k, in_word, hub_row;
  * marking (k_make_z_nz + k_mark_active + act / nz_in probes), probing (nz_in only), dense: steps 0-1, 2-3, 4-5 of
    test_walk_bit_parity at K >= 5, and the three feeds of test_step_counter_does_not_matter, whose x is 90 % zero rows so
    that the probes do skip;
  * G = 1 through launch_spmv_exact with a shifted zin (the hub row in the wave-per-row bin): every K = 1 case;
  * the empty slab (no make_z launch, an SpMM over a graph without links, r = 0): layout empty_mid, rank 1;
  * rwr_part_local_step / rwr_part_finish_step: every test here but test_end_to_end, which drives rwr_part_step as
    PartitionedRecommender does; test_fused_equals_split ties the two together;
  * the weighted branch at every tile width with lo > 0: the W cases.
"""
import math

import numpy as np
import pytest

from oracle.c_oracle import FlatGraph
from tests import part_cases as pc
from tests.slab_double import slab_partial

pytestmark = pytest.mark.gpu

NAN = float("nan")
C1 = 1 - pc.D

# every layout at G = 1, 8, 64 on VF; every G on the 3-slab layout of both graphs
CASES = sorted({("VF", lay, K) for lay in ("world3", "lo_64k", "in_word", "hub_row", "empty_mid", "whole") for K in (1, 5, 64)}
               | {(gname, "world3", K) for gname in ("VF", "W") for K in pc.KS})
case_ids = ["%s-%s-K%d" % c for c in CASES]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


class Rank:
    def __init__(self, g, lo, hi):
        from recommendersystems_amd import partitioned as pt
        local = pt.slab_graph(g, lo, hi)
        self.lo, self.hi = lo, hi
        self.F = FlatGraph(**local)
        self.be = pt.HipSlabBackend(local, lo, hi)
        expl = self.F.etype != 0
        self.in_deg = np.bincount(self.F.dst[expl], minlength=pc.N)       # in-links from in-slab sources
        # the path the slab graph takes (build.hip: every row's explicit raw weights equal)
        w, rp = self.F.w, self.F.rowptr
        self.uniform = all(len(set(w[rp[i]:rp[i + 1]][expl[rp[i]:rp[i + 1]]].tolist())) <= 1 for i in range(lo, hi))


@pytest.fixture(scope="module")
def ranks_of():
    cache = {}

    def get(gname, lname):
        if (gname, lname) not in cache:
            g = pc.graph(gname)
            full = FlatGraph(**g)
            ranks = [Rank(g, lo, hi) for lo, hi in pc.slabs(pc.layouts(g)[lname])]
            for rk in ranks:
                if pc.needs_dangling(rk.lo, rk.hi):
                    assert full.dangling[rk.lo:rk.hi].any()
                if rk.hi > rk.lo:
                    assert rk.be.graph.stats()["uniform_path"] == int(rk.uniform)
                    if gname == "VF":
                        assert rk.uniform
            if gname == "W":    # (a slab of ITEM rows alone has unit weights only: value-free even on this graph)
                assert [rk.uniform for rk in ranks][:2] == [False, False] and ranks[1].lo > 0
            cache[(gname, lname)] = ranks
        return pc.graph(gname), cache[(gname, lname)]
    yield get
    for ranks in cache.values():
        for rk in ranks:
            rk.be.graph.close()


def host(t, G):
    return t.cpu().numpy().reshape(-1, G)


def device_x(be, X):
    import torch
    return torch.from_numpy(np.ascontiguousarray(X).reshape(-1)).to(be.dev)


def check_partial(Yd, Yref, rk, K, what):
    """bits(Y_dev) == bits(Y_ref) over all n x G entries; no NaN left of the poison; padding columns and the rows no in-slab
    source reaches +0.0."""
    assert not np.isnan(Yd).any(), (what, "NaN in y: an unwritten entry, or a read outside the slab")
    bad = np.argwhere(bits(Yd) != bits(Yref))
    if len(bad):
        j, k = (int(v) for v in bad[0])
        raise AssertionError("%s: %d entries differ; first: row %d (slab [%d, %d), bitmap word %d bit %d, %d in-slab in-links) "
                             "column %d: device %r, reference %r" % (what, len(bad), j, rk.lo, rk.hi, j // 32, j % 32,
                                                                    int(rk.in_deg[j]), k, Yd[j, k], Yref[j, k]))
    assert (bits(Yd[:, K:]) == 0).all(), (what, "padding columns")
    assert (bits(Yd[rk.in_deg == 0]) == 0).all(), (what, "rows without an in-slab source")


def restart_depth(rows, G):
    """The most additions any one term goes through in k_slab_restart_partial / k_slab_restart_final: a thread adds
    ceil(rows / (512 * RL)) terms one after the other (512 blocks of RL = 256 / G rows), the block's tree has log2(RL)
    levels, the final kernel adds the 512 block sums one after the other.  All terms are >= 0, so every partial sum is <= the
    exact sum S and a sum of that shape is within ((1 + u) ** adds - 1) * S of S, u = 2 ** -53; the + 2 covers that bound's
    second-order part and the rounding of fsum."""
    RL = 256 // G
    return math.ceil(rows / (512 * RL)) + int(math.log2(RL)) + 512 + 2


def check_restart(rd, terms, rk, K, G, what):
    assert (terms >= 0).all()
    depth = restart_depth(rk.hi - rk.lo, G)
    for k in range(G):
        fs = math.fsum(terms[:, k])
        assert abs(float(rd[k]) - fs) <= depth * 2.0 ** -53 * fs, (what, "restart mass", k, float(rd[k]), fs)
    assert (rd[K:] == 0).all(), (what, "restart mass of the padding columns")


def local_checked(rk, x, y, r, K, G, what):
    """rwr_part_local_step of x into NaN-filled y, r; both checked against the reference of the device's own x."""
    y.fill_(NAN)
    r.fill_(NAN)
    rk.be.local_step(x, y, r)
    Yd, rd = host(y, G), r.cpu().numpy()
    Yref, terms = slab_partial(rk.F, rk.lo, rk.hi, C1, host(x, G))
    check_partial(Yd, Yref, rk, K, what)
    check_restart(rd, terms, rk, K, G, what)
    return Yd, rd


def checked_walk(ranks, seeds, steps, what):
    """rwr_part_begin on every rank, then `steps` steps of the exchange done on the host: partials and restart masses
    summed in rank order, the restart added at the seeds' rows, every rank handed ITS slab of the sum and NaN elsewhere."""
    K, G = len(seeds), pc.tile_width(len(seeds))
    state = [rk.be.begin(seeds, pc.D) for rk in ranks]
    assert all(rk.be.G == G for rk in ranks)
    for t in range(steps):
        Ysum, rsum = np.zeros((pc.N, G)), np.zeros(G)
        for q, (rk, (x, y, r)) in enumerate(zip(ranks, state)):
            Yd, rd = local_checked(rk, x, y, r, K, G, "%s step %d rank %d" % (what, t, q))
            Ysum += Yd
            rsum += rd
        Ysum[seeds, np.arange(K)] += rsum[:K]                       # rwr_part_finish_step, on the host copy
        for rk, (x, y, r) in zip(ranks, state):
            Xn = np.full((pc.N, G), NAN)
            Xn[rk.lo:rk.hi] = Ysum[rk.lo:rk.hi]
            x.copy_(device_x(rk.be, Xn))
    assert (Ysum[:, :K] > 0).any(axis=0).all() and not np.isnan(Ysum).any()
    return Ysum


@pytest.mark.parametrize("case", CASES, ids=case_ids)
def test_walk_bit_parity(ranks_of, case):
    """Six steps of a real walk: steps 0-1 mark, 2-3 probe only, 4-5 are dense (G >= 8 on a value-free slab; every other
    case takes its one form six times).  Every rank's partial is bitwise the reference's at every step, its restart mass
    within the derived bound."""
    gname, lname, K = case
    g, ranks = ranks_of(gname, lname)
    seeds = pc.seeds_for(g, pc.layouts(g)[lname], K)
    checked_walk(ranks, seeds, 6, "%s/%s K=%d" % case)


@pytest.mark.parametrize("case", CASES, ids=case_ids)
def test_step_counter_does_not_matter(ranks_of, case):
    """One sparse x (90 % zero rows, addends 60 binades apart, NaN outside the slab) fed right after rwr_part_begin (a marking
    step), after two steps (probing) and after four (dense): bitwise the reference each time."""
    gname, lname, K = case
    g, ranks = ranks_of(gname, lname)
    G = pc.tile_width(K)
    seeds = pc.seeds_for(g, pc.layouts(g)[lname], K)
    for q, rk in enumerate(ranks):
        Xs = pc.synthetic_x(rk.lo, rk.hi, K, G, seed=100 * K + q, g=g)
        seen = []
        for dummies in (0, 2, 4):
            x, y, r = rk.be.begin(seeds, pc.D)
            for _ in range(dummies):
                rk.be.local_step(x, y, r)
            Yd, _ = local_checked(rk, device_x(rk.be, Xs), y, r, K, G, "%s/%s K=%d rank %d after %d steps" % (case + (q, dummies)))
            seen.append(Yd)
        assert (bits(seen[0]) == bits(seen[1])).all() and (bits(seen[0]) == bits(seen[2])).all()
        if rk.hi > rk.lo and rk.F.nnz:
            assert (seen[0] != 0).any()


@pytest.mark.parametrize("case", CASES, ids=case_ids)
def test_fused_equals_split(ranks_of, case):
    """rwr_part_step on a stream of the caller's is rwr_part_local_step + rwr_part_finish_step: y2 == y off the seeds'
    entries, y2[s_k][k] == y[s_k][k] + r[k] at them, and finish_step on y gives y2 -- all bitwise."""
    import torch
    gname, lname, K = case
    g, ranks = ranks_of(gname, lname)
    G = pc.tile_width(K)
    seeds = pc.seeds_for(g, pc.layouts(g)[lname], K)
    for q, rk in enumerate(ranks):
        what = "%s/%s K=%d rank %d" % (case + (q,))
        _, y, r = rk.be.begin(seeds, pc.D)
        x = device_x(rk.be, pc.synthetic_x(rk.lo, rk.hi, K, G, seed=300 * K + q, g=g))
        Yd, rd = local_checked(rk, x, y, r, K, G, what)
        y2 = torch.full_like(y, NAN)
        torch.cuda.synchronize()
        side = torch.cuda.Stream(device=rk.be.dev)
        with torch.cuda.stream(side):
            rk.be.step(x, y2)
        side.synchronize()
        Y2 = host(y2, G)
        want = Yd.copy()
        want[seeds, np.arange(K)] = Yd[seeds, np.arange(K)] + rd[:K]
        assert (bits(Y2) == bits(want)).all(), what
        rk.be.finish_step(y, r)
        assert (bits(host(y, G)) == bits(Y2)).all(), what


@pytest.mark.parametrize("lname", ["world3", "empty_mid"])
@pytest.mark.parametrize("K", [5, 20])
def test_end_to_end(ranks_of, lname, K):
    """Ten steps of rwr_part_step with the exchange summed in rank order, then rwr_part_rank on the owners: lists and counts
    are the oracle's, scores within 1e-9 (the cross-rank sum re-associates), one owner per seed."""
    import torch
    g, ranks = ranks_of("VF", lname)
    G = pc.tile_width(K)
    seeds = pc.seeds_for(g, pc.layouts(g)[lname], K)
    state = [list(rk.be.begin(seeds, pc.D)[:2]) for rk in ranks]
    T = 10
    for it in range(T):
        for rk, (x, y) in zip(ranks, state):
            rk.be.step(x, y)
        ysum = torch.stack([st[1] for st in state]).sum(0)
        for rk, st in zip(ranks, state):
            if it + 1 == T:
                st[1].copy_(ysum)
            else:
                st[1].fill_(NAN)
                st[1][rk.lo * G:rk.hi * G] = ysum[rk.lo * G:rk.hi * G]
            st[0], st[1] = st[1], st[0]
    oi, os_, oc = FlatGraph(**g).recommend_batch(seeds, 0.15, T, 20)
    ids, sc, cnt = np.zeros_like(oi), np.zeros_like(os_), np.zeros_like(oc)
    owners = np.zeros(K, dtype=int)
    for rk, (x, y) in zip(ranks, state):
        i, s, c = rk.be.rank(x, 20)
        own = c >= 0
        assert (own == ((seeds >= rk.lo) & (seeds < rk.hi))).all()
        owners += own
        ids[own], sc[own], cnt[own] = i[own], s[own], c[own]
    assert (owners == 1).all()
    assert (cnt == oc).all() and (ids == oi).all()
    assert np.abs(sc - os_).max() <= 1e-9


@pytest.mark.parametrize("gname", ["VF", "W"])
def test_rebegin_on_warm_handles(ranks_of, gname):
    """rwr_part_begin again on handles that have walked: K = 64, then 3, then 20, other seeds each time.  The z buffer and the
    bitmaps only grow and the step counter starts over: two checked steps (marking ones where the slab has them) each."""
    g, ranks = ranks_of(gname, "world3")
    for salt, K in enumerate((64, 3, 20)):
        seeds = pc.seeds_for(g, pc.layouts(g)["world3"], K, salt=salt + 1)
        checked_walk(ranks, seeds, 2, "%s re-begin K=%d" % (gname, K))
