"""CPU-side check of the removal plan (recommendersystems_amd/csrc/remove_plan.h): which links rwr_graph_remove_links takes
out and how far every surviving link moves down -- the removed positions in ascending order, the new row pointers, the
shift function, the validation verdicts -- and of the device compaction's index arithmetic: the header's chunk slices,
segments, sparse/dense decision and dense destinations, with the segment copies of seg_copy.h, replayed lane by lane.
tests/cpp/remove_plan_check.cpp, built against the headers alone with the address and undefined-behaviour sanitizers,
compares all of it with a brute-force list-of-lists erase.  No library, no Python extension and no GPU are involved."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_remove_plan(tmp_path):
    exe = tmp_path / "remove_plan_check"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-I",
                           os.path.join(ROOT, "recommendersystems_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "remove_plan_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("0 failures"), r.stdout
