"""CPU-side check of the node append plan (recommendersystems_amd/csrc/node_append_plan.h): where rwr_graph_append_nodes puts
the new ITEM rows in the two ITEM orders -- the merge positions against std::stable_sort over the grown id set, ties
included -- the id key range, and the grown row pointers against a brute-force rebuild.
tests/cpp/node_append_plan_check.cpp is built against the headers alone, as a stand-alone program with the address and
undefined-behaviour sanitizers (the plan does size bookkeeping that can overrun silently).  No library, no Python extension
and no GPU are involved."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_node_append_plan(tmp_path):
    exe = tmp_path / "node_append_plan_check"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "recommendersystems_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "node_append_plan_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("0 failures"), r.stdout
