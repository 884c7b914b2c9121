"""CPU-side check of the host plan of the audience set entries (recommendersystems_amd/csrc/audience_set_plan.h): the ladder of
refusals in its documented order for both destinations (every later fault present, the earlier one wins) with the status of
each, the numbers the messages quote, the weight range at its edges, the merge of members that repeat in a set (list order; one
node in two sets), the (slot, row, weight) pairs across a tile-group boundary, and the exclusion tables -- two members of one
set under one slot, a member shared by sets of one group, a set that repeats, and their identity with audience_plan.h's table
for one-member sets.  tests/cpp/audience_set_plan_check.cpp, a program of its own built against the header alone with the
address and undefined-behaviour sanitizers, compares all of them with brute-force loops.  No library, no Python extension and
no GPU are involved."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_check(tmp_path, sanitize=True):
    exe = tmp_path / "audience_set_plan_check"
    flags = ["-fsanitize=address,undefined"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-I",
                           os.path.join(ROOT, "recommendersystems_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "audience_set_plan_check.cpp"), "-o", str(exe)])
    return exe


def test_audience_set_plan(tmp_path):
    exe = build_check(tmp_path)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("0 failures"), r.stdout
