"""The checks tests/test_gpu_build_edges.py runs on a built handle, and the child process of that file that reads row_order_x.

At default settings a graph of fewer than 50 000 nodes never reads row_order_x: launch_spmv_exact (spmv.hip) walks row_order
unless the step is two-phase (n >= spmv_big_n(), or RWR_SPMV_PHASES, which the shipped library reads once per process) or the
sweep is ready (value-free graph, n >= 50 000).  So the cases that put the row orders' sorts on their pass-count edges run here
once more, in a fresh interpreter started with RWR_SPMV_PHASES=1: the step then launches the binned kernel once per phase over
row_order_x (ITEM rows, then the others), which the counter spmv_binned_launches == 2 confirms.

    RWR_SPMV_PHASES=1 python tests/build_edges_child.py

prints BUILD_EDGES_PHASES_OK <case forms> on success."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import build_cases as bc                      # noqa: E402


def check_built(amd, G, norm, x, seed, ref, tag, binned_launches=None):
    """the three checks on a built handle: normalised arrays, stats, one deliver step (and, if given, how many launches of the
    row-binned kernel the step took)"""
    wn, dg = G.normalized()
    bad = np.nonzero(bc.bits(wn) != bc.bits(norm["w_norm"]))[0]
    assert bad.size == 0, (f"{tag}: w_norm differs at {bad.size} links, first {bad[0]}: got {float(wn[bad[0]]).hex()} "
                           f"want {float(norm['w_norm'][bad[0]]).hex()}")
    assert (np.asarray(dg) == norm["dangling"]).all(), f"{tag}: dangling differs at rows {np.nonzero(np.asarray(dg) != norm['dangling'])[0][:8]}"
    st = G.stats()
    assert (st["nnz"], st["uniform"], st["uniform_path"]) == (norm["nnz"], norm["uniform"], norm["uniform_path"]), \
        (tag, st["nnz"], st["uniform"], st["uniform_path"])
    m = amd.Model(G, bc.D, seed)
    m.rank = np.array(x, dtype=np.float64)
    G.reset_stats()
    m.deliverRanks()
    got = np.asarray(m.nextRank, dtype=np.float64)
    bad = np.nonzero(bc.bits(got) != bc.bits(ref))[0]
    assert bad.size == 0, (f"{tag}: nextRank differs at {bad.size} rows, first {bad[0]} (seed {seed}): got {float(got[bad[0]]).hex()} "
                           f"want {float(ref[bad[0]]).hex()}")
    if binned_launches is not None:
        assert G.stats()["spmv_binned_launches"] == binned_launches, (tag, G.stats()["spmv_binned_launches"])


def run_case(amd, case, form, binned_launches=None):
    norm, ref = case.reference(form)
    G = amd.Graph.from_flat(**case.flat_of(form))
    G.buildGraph()
    try:
        check_built(amd, G, norm, case.x, case.seed, ref, f"{case.name} {form}", binned_launches)
    finally:
        G.close()


def main():
    assert os.environ.get("RWR_SPMV_PHASES") == "1"
    import recommendersystems_amd as amd
    from recommendersystems_amd import _lib
    assert _lib.load().rwr_device_count() >= 1, "no gfx950 device: the HIP path cannot run"
    count = 0
    for case in bc.order_cases():
        types = case.flat["node_type"]
        assert (types == bc.NODE_ITEM).any() and (types != bc.NODE_ITEM).any()        # both phases hold rows: two launches
        for form in case.forms:
            # (a graph without explicit links has nothing to launch for: its step is checked, not counted)
            run_case(amd, case, form, binned_launches=2 if case.norm(form)["nnz"] else None)
            count += 1
    assert count > 0
    print("BUILD_EDGES_PHASES_OK", count)


if __name__ == "__main__":
    main()
