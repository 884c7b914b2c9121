"""Per-link tile masks for a batch's bitmap-probing steps: where a step of rwr_recommend_batch probes the frontier
bitmaps and walks every row, k_nz_transpose and k_entry_live answer "is this link's source live in tile t" once per link for
all tiles of the group, and k_spmm_entry_live reads the answer beside the index instead of probing the tile's bitmap per entry.
The bit is the one the probe would have read, so no result may move by a bit.

Every setting (read once per process) runs tests/entry_live_child.py in a fresh interpreter: RWR_ENTRY_LIVE=2 (the masks
whatever the graph's size -- the size rule keeps graphs of a few thousand nodes on the probe), RWR_ENTRY_LIVE=0 (the probe
everywhere), and RWR_ENTRY_LIVE=2 with RWR_ENTRY_LIVE_CAP_MB=0 (no group's masks fit the cap: the fallback).  The child sweeps
tile widths 8 to 64, groups of 1, 2 and 33 tiles (two slabs of masks) and T = 3, 4, 5, 10 on a handle an earlier batch has
dirtied, over graphs with rows of 0, 1, 15, 16, 17, 31, 32, 33, 65 and 130 in-links, and compares the forced run's width-16
results bitwise with the C restatement of the reference.  This file compares ids, counts and score bits between the settings
and checks rwr_stats.entry_live_launches.

What the counter must show follows from the plan (step_plan.h) for these seed sets, which hold an ITEM row -- only the last
step walks a tail list -- on graphs with two act steps and four probing steps: steps 0 and 1 walk frontier lists, so at
T = 10 exactly steps 2 and 3 read the masks; at T = 5 and 4 step 2 does (and step 3 unless it is the last); at T = 3 no step
probes every row, and the counter may stay 0."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KNOBS = ("RWR_ENTRY_LIVE", "RWR_ENTRY_LIVE_CAP_MB", "RWR_X_CLEAR", "RWR_CHAIN", "RWR_VALUE_FREE", "RWR_FRONTIER_LIST",
         "RWR_ACT_ITERS", "RWR_TAIL_ROWS", "RWR_TAIL_DEPTH", "RWR_SPMM", "RWR_BIG_N")
SETTINGS = {
    "forced": ({"RWR_ENTRY_LIVE": "2"}, True),
    "off": ({"RWR_ENTRY_LIVE": "0"}, False),
    "cap0": ({"RWR_ENTRY_LIVE": "2", "RWR_ENTRY_LIVE_CAP_MB": "0"}, False),
}


def run_child(tmp, tag, env_extra, oracle):
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(env_extra)
    path = os.path.join(str(tmp), tag + ".npz")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "entry_live_child.py"), path] + (["oracle"] if oracle else []),
                       capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    assert "ENTRY_LIVE_CHILD_OK" in p.stdout
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("entry_live")
    return {tag: run_child(tmp, tag, env, oracle) for tag, (env, oracle) in SETTINGS.items()}


def case_keys(run):
    return sorted(k[:-len("/stats")] for k in run if k.endswith("/stats"))


def test_masks_are_read_where_the_plan_says(runs):
    got = runs["forced"]
    keys = case_keys(got)
    assert len(keys) == 4 * 3 * 4 + 4 * 2
    total = 0
    for k in keys:
        live, spmm, listed = got[k + "/stats"].tolist()
        T = int(k.rsplit("/T", 1)[1])
        print("forced", k, "entry_live_launches, spmm_launches, frontier_list_launches:", live, spmm, listed)
        assert 0 <= live <= 2, k
        if T == 10:
            assert live == 2 and listed == 2, k          # steps 0 and 1 list, steps 2 and 3 read the masks
        elif T in (4, 5):
            assert live >= 1, k
        total += live
    assert total > 0
    # the oracle comparison ran for every batch of its width
    assert sum(k.endswith("/oracle") for k in got) == 3 * 4 + 2


@pytest.mark.parametrize("tag", ["off", "cap0"])
def test_probe_and_masks_agree_bitwise(tag, runs):
    got, ref = runs["forced"], runs[tag]
    assert case_keys(got) == case_keys(ref)
    for k in case_keys(got):
        for what in ("ids", "scores", "counts"):
            a, b = got[f"{k}/{what}"], ref[f"{k}/{what}"]
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), (tag, k, what)
        assert got[k + "/scores"].dtype == np.uint64
        live, spmm, listed = ref[k + "/stats"].tolist()
        print(tag, k, "entry_live_launches, spmm_launches, frontier_list_launches:", live, spmm, listed)
        assert live == 0, (tag, k)                       # RWR_ENTRY_LIVE=0, or no room under the cap: the bitmap probe
        # the same plan but for where the liveness comes from
        assert [spmm, listed] == got[k + "/stats"].tolist()[1:], (tag, k)
