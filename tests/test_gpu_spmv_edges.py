"""The single-seed SpMV step (spmv.hip: k_spmv_exact_binned and k_spmv_exact_hub; sweep.hip: the table kernels and
k_sweep_lds) on the crafted graphs of tests/spmv_cases.py: ONE Model.deliverRanks per case and form (value-free, weighted),
every row of nextRank bitwise against the list-order reference, then the rwr_stats counters that say which kernels served
the step -- the kernel the case was built for must have launched, the hub kernel as often as claimed, and in the child
processes the sweep's geometry must be the modelled one (in-process the CU count decides it: printed, not asserted).  The
sweep and hub cases also run a fresh Model.run(T), T = 1, 2, 3, against the C restatement of the reference.
tests/test_spmv_cases.py proves on the CPU that each case sits on the edge it was built for.

Default-knob cases run in this process; the others in one child per knob set (tests/spmv_edges_child.py).

Paths these cases cannot reach, stated so that they are not taken for covered:
  * blocks_for's cap of 16 384 workgroups, and with it the wave body's next-row prefetch loop and the strided loops of the
    group and lane bodies (a bin would need > 65 536 rows of >= 128 in-links, or > 1 M / 4 M rows of the others);
  * the lane body's 8-wide loop and its tails of 4 to 7 entries: the shipped library sends only rows of <= 3 in-links to it
    (RWR_GROUP_ROWS is read by the experiments build alone);
  * B > 512 source blocks (the sweep is then not taken) and entry streams past 2^32 word-rows (32-bit stream offsets);
  * a hub prefix other than 256 (RWR_HUB_PREFIX: experiments build only)."""
import os
import subprocess
import sys

import pytest

from tests import spmv_cases as sc
from tests import spmv_edges_child as child

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = sc.cases_for("default")
CHILD_SETS = [k for k in sc.KNOBS if k != "default"]


@pytest.fixture(scope="module")
def amd():
    import recommendersystems_amd as amd
    from recommendersystems_amd import _lib
    assert _lib.load().rwr_device_count() >= 1, "no gfx950 device: the HIP path cannot run"
    for knob in ("RWR_HUB_T", "RWR_SPMV_PHASES", "RWR_SWEEP", "RWR_SWEEP_MIN_N", "RWR_SWEEP_BN", "RWR_SWEEP_WGS", "RWR_HUB_SCAN",
                 "RWR_VALUE_FREE", "RWR_SPMM"):
        assert knob not in os.environ, f"{knob} is set: the in-process cases are built for the default knobs"
    return amd


@pytest.mark.parametrize("weighted", [False, True], ids=["valuefree", "weighted"])
@pytest.mark.parametrize("case", DEFAULT, ids=[c.name for c in DEFAULT])
def test_deliver_ranks_bitwise_on_crafted_graphs(amd, case, weighted):
    ref = sc.reference(case, weighted)
    ref.setflags(write=False)
    child.check_case(amd, case, weighted, "default", ref)


@pytest.mark.parametrize("knobs", CHILD_SETS)
def test_knob_dependent_cases_in_a_child_process(knobs):
    env = dict(os.environ)
    env.update(sc.KNOBS[knobs])
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "spmv_edges_child.py"), knobs], capture_output=True, text=True,
                       timeout=600, env=env)
    print(p.stdout[-6000:])
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    ok = [ln.split() for ln in p.stdout.splitlines() if ln.startswith("SPMV_EDGES_OK")]
    assert len(ok) == 1 and ok[0][1] == knobs and int(ok[0][2]) == 2 * len(sc.cases_for(knobs)) > 0, p.stdout[-1500:]
