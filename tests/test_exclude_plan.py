"""CPU-side check of the exclusion plan (recommendersystems_amd/csrc/exclude_plan.h): which raw links
rwr_recommend_restart_batch visits to mark the non-candidates of every vector -- the members' raw lists cut into segments of
at most 4096 links, ordered by slot, with one offset per tile group, and the validation verdicts of the exclusion sets.
tests/cpp/exclude_plan_check.cpp, built against the header alone with the address and undefined-behaviour sanitizers,
compares the segments with a direct walk over the members' lists.  No library, no Python extension and no GPU are involved."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exclude_plan(tmp_path):
    exe = tmp_path / "exclude_plan_check"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-I",
                           os.path.join(ROOT, "recommendersystems_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "exclude_plan_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("0 failures"), r.stdout
