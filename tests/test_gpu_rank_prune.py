"""Pruning the body of a batch's last step with a per-tile score bound (rank_bound.h): after the head's select
the thresholds give one float per source row and tile, and the selecting launch skips every body row whose sum of those floats
shows that no seed of the tile reaches its threshold there.  Results must be bitwise what they are without pruning.

Every setting of the knobs (read once per process) runs tests/rank_prune_child.py in a fresh interpreter.  The child compares
every case bitwise -- ids, scores, counts -- with the C restatement of the reference; this file compares the same arrays
bitwise with those of the RWR_RANK_PRUNE=0 child and checks the rank_pruned_rows / rank_fused_* counters of every call.  The
cases (see the child): tile widths 8, 16 and 32 with 45 seeds (a padded last tile each), 12 body rows that tie the threshold
exactly, every liked item in the body, a dangling seed, a tile with a threshold-0 slot (no pruning, and the group overflows
and falls back), body rows of more in-links than the bound is applied to, a weighted graph (pruning off), and -- with
RWR_RANK_FUSED_CAP=8 -- an overflow in every call, whose rerun is unpruned."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("RWR_RANK_FUSED", "RWR_RANK_FUSED_HEAD", "RWR_RANK_FUSED_CAP", "RWR_RANK_PRUNE", "RWR_VALUE_FREE")
CASES = ("tie-G8", "tie-G16", "tie-G32", "dangling", "tau0", "hot", "weighted")
PRUNED = ("tie-G8", "tie-G16", "tie-G32", "dangling", "hot")     # calls in which rows must have been skipped
FALL_BACK = ("tau0",)                                             # threshold 0: every row qualifies, the buffer overflows


def run_child(tmp, tag, env_extra):
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update({"RWR_RANK_FUSED": "2", "RWR_RANK_FUSED_HEAD": "13"})
    env.update(env_extra)
    path = os.path.join(str(tmp), tag + ".npz")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "rank_prune_child.py"), path], capture_output=True, text=True,
                       timeout=600, env=env)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    assert "RANK_PRUNE_CHILD_OK" in p.stdout
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("rank_prune")
    return {"off": run_child(tmp, "off", {"RWR_RANK_PRUNE": "0"}), "on": run_child(tmp, "on", {}),
            "cap8": run_child(tmp, "cap8", {"RWR_RANK_FUSED_CAP": "8"})}


@pytest.mark.parametrize("case", CASES)
def test_pruned_ranking_is_bitwise_the_unpruned_one(case, runs):
    off, on, cap8 = runs["off"], runs["on"], runs["cap8"]
    for what in ("ids", "scores", "counts"):
        k = f"{case}/{what}"
        for got in (on, cap8):
            assert got[k].dtype == off[k].dtype and np.array_equal(got[k], off[k]), k
    groups, fallbacks, pruned = on[case + "/stats"].tolist()
    print(case, "groups, fallbacks, pruned:", groups, fallbacks, pruned, "unpruned run:", off[case + "/stats"].tolist())
    assert off[case + "/stats"][2] == 0                           # RWR_RANK_PRUNE=0
    assert (groups, fallbacks) == ((0, 1) if case in FALL_BACK else (1, 0))
    assert off[case + "/stats"][:2].tolist() == [groups, fallbacks]
    if case in PRUNED:
        assert pruned > 0
    else:
        assert pruned == 0
    # a candidate buffer of 8 entries overflows in every call: the step runs again whole, and nothing counts as pruned
    assert cap8[case + "/stats"].tolist() == [0, 1, 0]
