"""Ranking inside the last step of a batch: the step runs over the first H rows of tail_rows[0], the select
ranks them, the rest of the step keeps only the rows that reach each seed's threshold, and a merge gives the lists.

Every setting of the knobs (read once per process) runs tests/rank_fused_child.py in a fresh interpreter.  The child
compares every case bitwise -- ids, scores, counts -- with the C restatement of the reference; this file compares the same
arrays bitwise with those of the RWR_RANK_FUSED=0 child and checks, from the rank_fused_groups / rank_fused_fallbacks counters,
that each call took the path it should.  The cases (see the child): three groups of 25 items with identical in-lists at the
top of the in-degree order, so that a head of 13 rows ends inside a tie group and top_n = 5, 30, 60 cut through one; seeds
that like 30 cold items nobody else likes (far above the threshold, outside the head, excluded); seeds that like a whole
tie group, whose head therefore holds fewer than top_n candidates (threshold 0: without overflow on the 1500-item graph,
with overflow on the 6000-item one); G = 8, 16, 32 with 13 seeds (padded slots), duplicate seeds, a dangling seed; raw
weights that differ inside a row (the weighted kernels); and the calls the split must leave alone: an ITEM seed, T = 1..4,
top_n = 1025, a negative weight."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("RWR_RANK_FUSED", "RWR_RANK_FUSED_HEAD", "RWR_RANK_FUSED_CAP", "RWR_VALUE_FREE")
# calls the split does not apply to: they keep the path of before
UNSPLIT = ("tie-item-seed", "tie-T1", "tie-T2", "tie-T3", "tie-T4", "tie-top1025", "negative")


def run_child(tmp, tag, env_extra):
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(env_extra)
    path = os.path.join(str(tmp), tag + ".npz")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "rank_fused_child.py"), path], capture_output=True, text=True,
                       timeout=600, env=env)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    assert "RANK_FUSED_CHILD_OK" in p.stdout
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def unfused(tmp_path_factory):
    res = run_child(tmp_path_factory.mktemp("rank_fused"), "off", {"RWR_RANK_FUSED": "0"})
    for k, v in res.items():
        if k.endswith("/fused"):
            assert v.tolist() == [0, 0], (k, v)
    return res


# env, cases that must fall back (all others that the split applies to must not).  The 6000-item graph falls back under every
# setting with rows beyond the head: its ~1000 random likes leave most items without a link and some seeds (150, 180, 190)
# in components of a few nodes, so that their head's top_n-th score, the threshold, is 0 and the thousands of items with
# score 0 all reach it -- more than a candidate buffer holds.
SETTINGS = {
    "default-head": ({}, ("big-top5",)),
    "head-13": ({"RWR_RANK_FUSED_HEAD": "13"}, ("big-top5",)),
    "head-1": ({"RWR_RANK_FUSED_HEAD": "1"}, ("big-top5",)),
    "head-all-rows": ({"RWR_RANK_FUSED_HEAD": "1000000"}, ()),
    "head-13-weighted": ({"RWR_RANK_FUSED_HEAD": "13", "RWR_VALUE_FREE": "0"}, ("big-top5",)),
    "capacity-8": ({"RWR_RANK_FUSED_HEAD": "13", "RWR_RANK_FUSED_CAP": "8"}, None),   # None: every split call falls back
}
# (by default the split starts at 2^18 ITEM rows; RWR_RANK_FUSED=2 takes it on these graphs of a few thousand nodes)
SETTINGS = {k: (dict(env, RWR_RANK_FUSED="2"), fb) for k, (env, fb) in SETTINGS.items()}


@pytest.mark.parametrize("setting", list(SETTINGS), ids=list(SETTINGS))
def test_fused_ranking_is_bitwise_the_unfused_one(setting, unfused, tmp_path):
    env, fall_back = SETTINGS[setting]
    got = run_child(tmp_path, "on", env)
    assert set(got) == set(unfused)
    for k in sorted(got):
        name, what = k.rsplit("/", 1)
        if what != "fused":
            assert got[k].dtype == unfused[k].dtype and np.array_equal(got[k], unfused[k]), (setting, k)
            continue
        groups, fallbacks = got[k].tolist()
        if name in UNSPLIT:
            assert (groups, fallbacks) == (0, 0), (setting, name, groups, fallbacks)
        elif fall_back is None or name in fall_back:
            assert (groups, fallbacks) == (0, 1), (setting, name, groups, fallbacks)     # (one tile group per call)
        else:
            assert (groups, fallbacks) == (1, 0), (setting, name, groups, fallbacks)
