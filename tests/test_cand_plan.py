"""CPU-side check of the typed recommendation's host plan (recommendersystems_amd/csrc/cand_plan.h): the block geometry and
block offsets of the candidate-list compaction (the one host model, filter_plan.h's, without a pool), and which cached list
serves a call (hit, rebuild in place, which entry a new type evicts -- over sequences with a growing node count).  The verdicts
on the arguments of rwr_recommend_typed_batch are tests/test_typed_call.py's.  tests/cpp/cand_plan_check.cpp, a program of its
own built against the headers alone with the address and undefined-behaviour sanitizers, compares both with brute-force loops.
No library, no Python extension and no GPU are involved."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cand_plan(tmp_path):
    exe = tmp_path / "cand_plan_check"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-I",
                           os.path.join(ROOT, "recommendersystems_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "cand_plan_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("0 failures"), r.stdout
