"""A batch's last steps walk row lists up to four levels deep, and a step's seed-row chain runs only where the seed's row
can still reach a row the ranking reads.  The results must stay bitwise the reference's -- on bipartite
like-graphs (where four levels are taken, asserted through the launch counters) and on graphs that are not, with seeds whose
links make the chains of steps T, T - 1 or T - 2 run, dangling seeds, T = 1 .. 10, tile widths 8-64 and after
rwr_graph_update_links -- and equal to what the full-row steps give (RWR_TAIL_ROWS=0) and what the two-level tail gives
(RWR_TAIL_DEPTH=2), each in a fresh process (tests/tail_depth_child.py)."""
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
    from tests import tail_depth_child
    assert _lib.load().rwr_device_count() >= 1, "no gfx950 device: the HIP path cannot run"
    return tail_depth_child.run_all(amd)


def run_child(env_extra):
    env = dict(os.environ)
    env.update(env_extra)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tail_depth_child.py")], capture_output=True,
                       text=True, env=env, cwd=ROOT, timeout=1200)
    assert p.returncode == 0, f"child failed ({env_extra}):\n{p.stdout[-4000:]}\n{p.stderr[-4000:]}"
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("TAIL_DEPTH_CHILD_OK")]
    assert line, p.stdout[-2000:]
    _, cases, digest = line[-1].split()
    return int(cases), digest


def test_tail_depth_bitwise_vs_oracle(in_process):
    cases, _ = in_process
    assert cases > 700


@pytest.mark.parametrize("env", [{"RWR_TAIL_ROWS": "0"}, {"RWR_TAIL_DEPTH": "2"}],
                         ids=lambda e: ",".join(f"{k}={v}" for k, v in e.items()))
def test_tail_depth_same_results_in_fresh_process(in_process, env):
    assert run_child(env) == in_process
