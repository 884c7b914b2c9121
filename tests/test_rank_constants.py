"""The dispatch constants of the ranking stage, read out of the sources.  tests/test_gpu_rank_paths.py builds its
boundary cases (bins of exactly SEL_CAP members, one or several select row blocks, the sort's block carry, the small
path's edge) around these values: a retune that moves one of them would quietly move those cases off their boundary.
CPU only."""
import os
import re

import pytest

from tests.test_gpu_rank_paths import EXPECTED_CONSTANTS

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "recommendersystems_amd", "csrc")

WHERE = {
    "SEL_MAX_K": "rank_keys.h", "SEL_CAP": "rank_keys.h", "SEL_SLOTS": "rank_keys.h", "SEL_ROWS_PER_BLOCK": "rank_keys.h",
    "SEL_FUSED_LEVELS": "rank_keys.h", "SORT_CHUNK": "sort.hip", "SMALL_SORT_MAX": "sort_small.h",
    "SM_MAX_ITEMS": "small.hip",
}


def read_constant(name: str) -> int:
    with open(os.path.join(CSRC, WHERE[name])) as f:
        src = f.read()
    found = re.findall(r"constexpr\s+[\w:]+\s+" + name + r"\s*=\s*([^;]+);", src)
    assert len(found) == 1, f"{name}: expected one definition in {WHERE[name]}, found {len(found)}"
    expr = found[0].strip()
    if name == "SORT_CHUNK":      # SORT_BLOCK * SORT_ITEMS
        vals = {k: int(v) for k, v in re.findall(r"constexpr\s+int\s+(SORT_BLOCK|SORT_ITEMS)\s*=\s*(\d+)\s*;", src)}
        return vals["SORT_BLOCK"] * vals["SORT_ITEMS"] if expr == "SORT_BLOCK * SORT_ITEMS" else int(expr)
    return int(expr)


@pytest.mark.parametrize("name", sorted(WHERE))
def test_rank_dispatch_constant_is_where_the_gpu_cases_expect_it(name):
    got = read_constant(name)
    assert got == EXPECTED_CONSTANTS[name], (
        f"{name} is {got} in {WHERE[name]}, but tests/test_gpu_rank_paths.py builds its boundary cases around "
        f"{EXPECTED_CONSTANTS[name]}: move those cases onto the new boundary, then update EXPECTED_CONSTANTS there")


def test_select_slots_hold_the_worst_collection():
    """k - 1 entries above the k-th entry's bin plus a bin of SEL_CAP members must fit the candidate slots."""
    assert read_constant("SEL_MAX_K") - 1 + read_constant("SEL_CAP") <= read_constant("SEL_SLOTS")
