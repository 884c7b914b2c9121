"""CPU-side check of the filtered recommendation's host plan (recommendersystems_amd/csrc/filter_plan.h): the bitmap and block
geometry of the candidate-list build (n = 0, 1, 31, 32, 33, 255, 256, 257 and beyond one scan chunk), the bitmap, block offsets
and list of pools in any order and with duplicates.  (The verdicts on the arguments of rwr_recommend_filtered_batch and
rwr_recommend_filtered_positions_batch are tests/test_typed_call.py's.)  tests/cpp/filter_plan_check.cpp, a program of its own built
against the header alone with the address and undefined-behaviour sanitizers, compares all of them with brute-force loops.  No
library, no Python extension and no GPU are involved."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_filter_plan(tmp_path):
    exe = tmp_path / "filter_plan_check"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-I",
                           os.path.join(ROOT, "recommendersystems_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "filter_plan_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("0 failures"), r.stdout
