"""No clear of the rank matrix on the frontier-list path: a ranking-only batch whose seed-row chain is the
role-specialised fold starts from whatever an earlier call left in X, and the fold beside step 2 reads step 1's listed
output through the frontier bitmap (k_seed_chain_roles<G, MASK = true>).  Results must not move by a bit.

Every setting (read once per process) runs tests/x_clear_child.py in a fresh interpreter.  The child ranks one seed set after
another one has dirtied the handle's workspace and compares ids, scores and counts bitwise with the C restatement of the
reference, for T in {2, 3, 4, 6, 10} -- step 1 is the last step, a tail-list step, a frontier-list step in turn.  This file
compares the same arrays bitwise with those of a fresh handle under RWR_X_CLEAR=1 (the cleared, unmasked path) and checks
through rwr_stats.x_clear_skipped that the clear was skipped exactly where it may be: with the fold (RWR_CHAIN=3, both with
the value-free kernels and with the weighted ones, RWR_VALUE_FREE=0), not with RWR_X_CLEAR=1, and not with the binade scan,
which this batch of 43 seeds takes by default and which has no masked form."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("RWR_X_CLEAR", "RWR_CHAIN", "RWR_VALUE_FREE", "RWR_FRONTIER_LIST", "RWR_ACT_ITERS", "RWR_TAIL_ROWS", "RWR_SPMM")
T_VALUES = (2, 3, 4, 6, 10)
SETTINGS = {
    "fold": {"RWR_CHAIN": "3"},
    "fold-cleared": {"RWR_CHAIN": "3", "RWR_X_CLEAR": "1"},
    "fold-weighted": {"RWR_CHAIN": "3", "RWR_VALUE_FREE": "0"},
    "fold-weighted-cleared": {"RWR_CHAIN": "3", "RWR_VALUE_FREE": "0", "RWR_X_CLEAR": "1"},
    "scan": {},
}
REFERENCE = {"fold": "fold-cleared", "fold-weighted": "fold-weighted-cleared", "scan": "fold-cleared"}
SKIPS = {"fold": 1, "fold-weighted": 1, "scan": 0, "fold-cleared": 0, "fold-weighted-cleared": 0}   # per call of one tile group


def run_child(tmp, tag, env_extra):
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(env_extra)
    path = os.path.join(str(tmp), tag + ".npz")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "x_clear_child.py"), path], capture_output=True, text=True,
                       timeout=600, env=env)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    assert "X_CLEAR_CHILD_OK" in p.stdout
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("x_clear")
    return {tag: run_child(tmp, tag, env) for tag, env in SETTINGS.items()}


SETS = ("mixed", "users")


@pytest.mark.parametrize("tag", sorted(REFERENCE))
def test_stale_rank_matrix_changes_no_bit(tag, runs):
    got, ref = runs[tag], runs[REFERENCE[tag]]
    for name in SETS:
        for T in T_VALUES:
            for what in ("ids", "scores", "counts"):
                k = f"{name}/T{T}/{what}"
                assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), (tag, k)
            skipped, listed, chains = got[f"{name}/T{T}/stats"].tolist()
            print(tag, name, "T", T, "x_clear_skipped, frontier_list_launches, chain_launches:", skipped, listed, chains)
            assert skipped == SKIPS[tag], (tag, name, T)
            # the same plan but for the mask: as many listed launches and chains as on the cleared path
            if tag != "scan":
                assert [listed, chains] == ref[f"{name}/T{T}/stats"][1:].tolist(), (tag, name, T)
        # T = 6, 10: steps 0 and 1 walk their frontier lists and step 2 runs a chain, which is the masked fold wherever the
        # clear was skipped; T = 3 with an ITEM seed: the same beside the last step
        for T in (6, 10):
            assert got[f"{name}/T{T}/stats"][1] == 2 and got[f"{name}/T{T}/stats"][2] >= 3, (tag, name, T)
    assert got["mixed/T3/stats"].tolist()[1:] == [2, 3], tag
    # without an ITEM seed step 1 is a tail-list step at T = 3: nothing lists
    assert got["users/T3/stats"][1] == 0, tag


@pytest.mark.parametrize("tag", ["fold-cleared", "fold-weighted-cleared"])
def test_x_clear_knob_restores_the_clear(tag, runs):
    for name in SETS:
        for T in T_VALUES:
            assert runs[tag][f"{name}/T{T}/stats"][0] == 0
        assert runs[tag][f"{name}/T10/stats"][1] == 2
