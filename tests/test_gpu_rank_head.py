"""The size of the exact head of a batch's last step ("A smaller head"): whatever RWR_RANK_FUSED_HEAD says, the
lists are bitwise those of the reference and of a run without the split, and the counters say which way each call went.

Every head size runs tests/rank_head_child.py in a fresh interpreter (the library reads its environment once per process) with
RWR_RANK_FUSED=2; the child compares every case bitwise -- ids, scores, counts -- with the C restatement of the reference, this
file compares the same arrays with those of the RWR_RANK_FUSED=0 child.  The graph (see the child): 100 hot items open the
in-degree order, 7 900 cold ones follow, 40 seeds that like cold items only, T = 6, top_n = 100; two tiles at G = 32, five at
G = 8, and 36 seeds with padded slots.  Heads:
  1, 64          fewer than top_n head entries: threshold 0, the tile is not pruned, every row qualifies, the candidate buffer
                 overflows and the group falls back;
  100            exactly top_n head entries per seed, a positive threshold: rows are pruned, no fallback;
  n_items - 1    a body of one row;
  n_items        no body at all.
The host-only test checks the study tool's tiling (tools/rank_head_study.py: deal_tiles) against the rule of
upload_seed_slots: in-degree-descending, stable, round-robin over the tiles."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("RWR_RANK_FUSED", "RWR_RANK_FUSED_HEAD", "RWR_RANK_FUSED_CAP", "RWR_RANK_PRUNE", "RWR_VALUE_FREE")
CASES = ("G32", "G8", "G8-padded")
N_ITEMS = 8000
HEADS = (1, 64, 100, N_ITEMS - 1, N_ITEMS)


def run_child(tmp, tag, env_extra):
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(env_extra)
    path = os.path.join(str(tmp), tag + ".npz")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "rank_head_child.py"), path], capture_output=True, text=True,
                       timeout=600, env=env)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    assert "RANK_HEAD_CHILD_OK" in p.stdout
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def unsplit(tmp_path_factory):
    return run_child(tmp_path_factory.mktemp("rank_head_off"), "off", {"RWR_RANK_FUSED": "0"})


@pytest.mark.gpu
@pytest.mark.parametrize("head", HEADS)
def test_any_head_gives_the_unsplit_ranking_bitwise(head, unsplit, tmp_path):
    got = run_child(tmp_path, f"h{head}", {"RWR_RANK_FUSED": "2", "RWR_RANK_FUSED_HEAD": str(head)})
    for case in CASES:
        for what in ("ids", "scores", "counts"):
            k = f"{case}/{what}"
            assert got[k].dtype == unsplit[k].dtype and np.array_equal(got[k], unsplit[k]), k
        groups, fallbacks, pruned = got[case + "/stats"].tolist()
        print(head, case, "groups, fallbacks, pruned:", groups, fallbacks, pruned)
        assert unsplit[case + "/stats"].tolist() == [0, 0, 0]         # RWR_RANK_FUSED=0
        if head < 100:
            assert (groups, fallbacks, pruned) == (0, 1, 0)           # threshold 0: nothing pruned, overflow, the step whole
        elif head == 100:
            assert (groups, fallbacks) == (1, 0) and pruned > 0
        elif head == N_ITEMS - 1:
            assert (groups, fallbacks) == (1, 0) and pruned >= 0
        else:
            assert (groups, fallbacks, pruned) == (1, 0, 0)           # no body: nothing to prune


def load_tool():
    spec = importlib.util.spec_from_file_location("rank_head_study", os.path.join(ROOT, "tools", "rank_head_study.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def deal_by_the_rule(seeds, indeg, G):
    """upload_seed_slots, restated entry by entry"""
    K = len(seeds)
    ntiles = -(-K // G)
    order = list(range(K))
    # a stable insertion sort, highest in-degree first
    for i in range(1, K):
        j = i
        while j > 0 and indeg[seeds[order[j - 1]]] < indeg[seeds[order[j]]]:
            order[j - 1], order[j] = order[j], order[j - 1]
            j -= 1
    slots = [-1] * (ntiles * G)
    for r in range(K):
        slots[(r % ntiles) * G + r // ntiles] = seeds[order[r]]
    return np.array(slots).reshape(ntiles, G)


@pytest.mark.parametrize("K,G", [(1, 8), (8, 8), (40, 32), (45, 8), (64, 32), (97, 16)])
def test_study_tiles_are_dealt_as_the_library_deals_them(K, G):
    tool = load_tool()
    rng = np.random.default_rng(K * 100 + G)
    indeg = rng.integers(0, 6, size=500)               # few distinct values: many equal in-degrees, the order must be stable
    seeds = rng.integers(0, 500, size=K)               # duplicates allowed, as in a batch
    got = tool.deal_tiles(seeds, indeg, G)
    want = deal_by_the_rule(seeds.tolist(), indeg.tolist(), G)
    assert got.shape == want.shape and np.array_equal(got, want)
    # every tile's leading slot holds one of the ntiles heaviest seeds; padded slots are the last ones of the last tiles
    ntiles = want.shape[0]
    top = np.sort(indeg[seeds])[::-1][:ntiles]
    assert sorted(indeg[got[:, 0]].tolist(), reverse=True) == top.tolist()
    assert (got >= 0).sum() == K
