"""CPU-side check of the append plan (recommendersystems_amd/csrc/append_plan.h): where rwr_graph_append_links puts the
new links and how far every resident link moves -- the stable order of the new links by source, the distinct sources with
their counts, the breakpoints of the shift function with their running sums, new_index_out, and the validation verdicts.
tests/cpp/append_plan_check.cpp, built against the header alone with the address and undefined-behaviour sanitizers,
compares the plan with a brute-force list-of-lists append.  No library, no Python extension and no GPU are involved."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_append_plan(tmp_path):
    exe = tmp_path / "append_plan_check"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-I",
                           os.path.join(ROOT, "recommendersystems_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "append_plan_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("0 failures"), r.stdout
