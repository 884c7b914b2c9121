"""The row lists of a batch's pruned last step: k_sel_bound_compact turns the keep bits of the body rows into one
list per tile in ONE pass -- a workgroup takes a span of 2 048 positions of tail_rows[0], reads each keep word once for the 32
tiles of its block, and reserves each tile's places with one atomicAdd.  The lists must hold exactly the kept rows: results are
bitwise those of the oracle (checked in the child, tests/bound_compact_child.py) and of RWR_RANK_PRUNE=0, and the
(row, tile) pairs skipped are as many as before the kernel was rewritten.

Cases (graphs in the child): a body of 2 487 rows -- one span and 439 rows -- whose second span has no kept row in a tile that
prunes; a tile that keeps every row (a threshold-0 slot) beside tiles that prune; 39 tiles, two blocks of 32, with whole-list
tiles in the second block and in the first; a body of 15 012 rows, eight spans, the last of them without a kept row.

PARENT_PRUNED: rank_pruned_rows of the same calls at the parent commit (the per-wave compaction), recorded on an MI355X."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("RWR_RANK_FUSED", "RWR_RANK_FUSED_HEAD", "RWR_RANK_FUSED_CAP", "RWR_RANK_PRUNE", "RWR_VALUE_FREE")
PARENT_PRUNED = {"pruned-tiles": 11649, "one-kept-whole": 10042, "two-blocks": 48095, "long": 42911}
BODY = {"pruned-tiles": 2487, "one-kept-whole": 2487, "two-blocks": 2487, "long": 15012}       # rows past the head of 13
BARE = {"pruned-tiles": 500, "one-kept-whole": 500, "two-blocks": 500, "long": 5000}            # ... of them without in-links
TILES = {"pruned-tiles": 6, "one-kept-whole": 6, "two-blocks": 39, "long": 3}
WHOLE = {"pruned-tiles": 0, "one-kept-whole": 1, "two-blocks": 12, "long": 0}    # tiles with a threshold-0 slot: nothing pruned


def run_child(tmp, tag, env_extra):
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update({"RWR_RANK_FUSED": "2", "RWR_RANK_FUSED_HEAD": "13"})
    env.update(env_extra)
    path = os.path.join(str(tmp), tag + ".npz")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bound_compact_child.py"), path], capture_output=True,
                       text=True, timeout=600, env=env)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    assert "BOUND_COMPACT_CHILD_OK" in p.stdout
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("bound_compact")
    return {"off": run_child(tmp, "off", {"RWR_RANK_PRUNE": "0"}), "on": run_child(tmp, "on", {})}


@pytest.mark.parametrize("case", sorted(PARENT_PRUNED))
def test_compacted_lists_hold_the_kept_rows(case, runs):
    off, on = runs["off"], runs["on"]
    for what in ("ids", "scores", "counts"):
        k = f"{case}/{what}"
        assert on[k].dtype == off[k].dtype and np.array_equal(on[k], off[k]), k
    groups, fallbacks, pruned, tile_group = on[case + "/stats"].tolist()
    print(case, "groups, fallbacks, pruned:", groups, fallbacks, pruned, "unpruned run:", off[case + "/stats"].tolist())
    assert tile_group >= TILES[case]                              # one group: its tiles share the compaction's launch
    assert (groups, fallbacks) == (1, 0) and off[case + "/stats"][:3].tolist() == [1, 0, 0]
    # a whole-list tile skips nothing, a pruning tile at least the rows without in-links, which fill the last span(s)
    assert (TILES[case] - WHOLE[case]) * BARE[case] <= pruned <= (TILES[case] - WHOLE[case]) * BODY[case]
    assert pruned == PARENT_PRUNED[case]
