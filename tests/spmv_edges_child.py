"""Child process of tests/test_gpu_spmv_edges.py, and the one routine both share: librwr reads its knobs from the
environment ONCE per process, so the cases of tests/spmv_cases.py that are built for a knob set other than the default run in
a fresh interpreter started with that set (RWR_HUB_T, RWR_SPMV_PHASES, RWR_SWEEP_MIN_N, RWR_SWEEP_BN, RWR_SWEEP_WGS).

    python tests/spmv_edges_child.py <knob set>

runs every case of the set in both forms and prints SPMV_EDGES_OK <knob set> <cases> on success."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import spmv_cases as sc                      # noqa: E402

GEOMETRY = ("sweep_k", "sweep_blocks", "sweep_wgs", "sweep_partial")
RUN_STEPS = (1, 2, 3)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def check_case(amd, case, weighted, knobs, ref):
    """ONE deliverRanks on the case's rank vector: all rows bitwise against `ref`, then the counters against the case's
    claims; for the sweep and hub cases a fresh Model.run(T), T = 1, 2, 3, against the C restatement of the reference (zout,
    the act / nz_out masks of a fresh run's first steps, the step-to-step hand-over).  Returns a line for the log."""
    from oracle.c_oracle import FlatGraph
    cl = case.claims
    flat = case.flat(weighted)
    tag = f"{case.name} [{cl['branch']}] {knobs} {'weighted' if weighted else 'value-free'}"
    G = amd.Graph.from_flat(**flat)
    G.buildGraph()
    try:
        assert G.stats()["uniform_path"] == (0 if weighted else 1), tag
        m = amd.Model(G, case.d, case.seed)
        m.rank = case.x.copy()
        G.reset_stats()
        m.deliverRanks()
        got = np.asarray(m.nextRank, dtype=np.float64).copy()
        st = G.stats()
        runs = {}
        if cl.get("run_check"):
            for T in RUN_STEPS:
                mm = amd.Model(G, case.d, case.seed)
                mm.run(T)
                runs[T] = np.asarray(mm.rank, dtype=np.float64).copy()
    finally:
        G.close()
    diff = np.nonzero(bits(got) != bits(ref))[0]
    assert diff.size == 0, (f"{tag}: {diff.size} rows differ, first row {diff[0]} (seed {case.seed}, in-links {case.in_deg[diff[0]]}): "
                            f"got {float(got[diff[0]]).hex()} want {float(ref[diff[0]]).hex()}")
    counters = {k: st[k] for k in ("spmv_sweep_launches", "spmv_hub_launches", "spmv_binned_launches") + GEOMETRY}
    note = f"{tag}: {counters}"
    print(note, flush=True)
    if cl["kernel"] == "sweep" and not weighted:
        assert st["spmv_sweep_launches"] == 1, note
        assert (st["spmv_binned_launches"] >= 1) == bool(cl.get("binned_beside")), note
    else:
        assert st["spmv_sweep_launches"] == 0 and st["spmv_binned_launches"] >= 1, note
        assert all(st[k] == 0 for k in GEOMETRY), note
    assert st["spmv_hub_launches"] == cl["hub_launches"][1 if weighted else 0], note
    if "geometry" in cl and not weighted:                 # (in-process, where the CU count decides, it is printed only)
        want = cl["geometry"]
        assert (st["sweep_k"], st["sweep_blocks"], st["sweep_wgs"], st["sweep_partial"]) == \
            (want["k"], want["blocks"], want["wgs"], want["partial"]), note
    if runs:
        F = FlatGraph(**flat)
        for T, r in runs.items():
            want, _ = F.model_run(case.d, case.seed, 0, T)
            bad = np.nonzero(bits(r) != bits(want))[0]
            assert bad.size == 0, (f"{tag}: Model.run({T}): {bad.size} rows differ, first row {bad[0]}: "
                                   f"got {float(r[bad[0]]).hex()} want {float(want[bad[0]]).hex()}")
    return note


def main():
    knobs = sys.argv[1]
    for k, v in sc.KNOBS[knobs].items():
        assert os.environ.get(k) == v, (k, os.environ.get(k), v)
    import recommendersystems_amd as amd
    from recommendersystems_amd import _lib
    assert _lib.load().rwr_device_count() >= 1, "no gfx950 device: the HIP path cannot run"
    count = 0
    for case in sc.cases_for(knobs):
        for weighted in (False, True):
            ref = sc.reference(case, weighted)
            check_case(amd, case, weighted, knobs, ref)
            count += 1
    assert count > 0
    print("SPMV_EDGES_OK", knobs, count)


if __name__ == "__main__":
    main()
