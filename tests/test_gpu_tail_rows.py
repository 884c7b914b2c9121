"""A batch's last two steps produce only the rows the ranking reads: the ITEM rows at step T, the sources
of the ITEM rows' in-links at step T - 1 (unless a seed of the tile group is an ITEM, whose last chain reads every row).
The results must stay bitwise the reference's -- on graphs that are not bipartite, at every tile width, for T = 1 .. 10,
with and without ITEM seeds, and after rwr_graph_update_links has changed which rows link into ITEM rows -- and equal to
what the full-row steps give (RWR_TAIL_ROWS=0) and what the plain SpMM kernel gives (RWR_SPMM=0), each in a fresh process
(tests/tail_rows_child.py)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def in_process():
    import recommendersystems_amd as amd
    from recommendersystems_amd import _lib
    from tests import tail_rows_child
    assert _lib.load().rwr_device_count() >= 1, "no gfx950 device: the HIP path cannot run"
    return tail_rows_child.run_all(amd)


def run_child(env_extra):
    env = dict(os.environ)
    env.update(env_extra)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tail_rows_child.py")], capture_output=True,
                       text=True, env=env, cwd=ROOT, timeout=1200)
    assert p.returncode == 0, f"child failed ({env_extra}):\n{p.stdout[-4000:]}\n{p.stderr[-4000:]}"
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("TAIL_ROWS_CHILD_OK")]
    assert line, p.stdout[-2000:]
    _, cases, digest = line[-1].split()
    return int(cases), digest


def test_tail_rows_bitwise_vs_oracle(in_process):
    cases, _ = in_process
    assert cases > 300


@pytest.mark.parametrize("env", [{"RWR_TAIL_ROWS": "0"}, {"RWR_SPMM": "0"}],
                         ids=lambda e: ",".join(f"{k}={v}" for k, v in e.items()))
def test_tail_rows_same_results_in_fresh_process(in_process, env):
    assert run_child(env) == in_process
