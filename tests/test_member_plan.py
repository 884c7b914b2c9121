"""CPU-side check of the typed ends' host plan (recommendersystems_amd/csrc/member_plan.h): the (slot, member) pairs whose own
rows rwr_recommend_restart_typed_batch marks -- slot order, group offsets, empty padding slots, repeated members, empty sets,
group boundaries.  (The argument verdicts that rwr_recommend_typed_eval_batch and rwr_recommend_restart_typed_batch add to
those of the entries they extend are tests/test_typed_call.py's.)  tests/cpp/member_plan_check.cpp, a program of its own built against the headers alone with
the address and undefined-behaviour sanitizers, compares them with brute-force loops.  No library, no Python extension and no
GPU are involved."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_member_plan(tmp_path):
    exe = tmp_path / "member_plan_check"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-I",
                           os.path.join(ROOT, "recommendersystems_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "member_plan_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("0 failures"), r.stdout
