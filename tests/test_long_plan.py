"""CPU-side check of the host plan of the long-list destination (recommendersystems_amd/csrc/long_plan.h): the collect
capacity and the run / pass tables for every collected count from 0 to 3R + 1 and at the capacities of top_n = 1 025 and
65 536, the buffer that holds the result, the merge-path partition and the ranged merge against std::merge on crafted runs
(all equal, strictly interleaved, one run empty, lengths that differ by one), the host model of the whole selection against
std::stable_sort on keys with heavy duplication under several arrival orders of the collect, the tile-by-tile split, and the
ladders of both long entries with every fault present, one repaired at a time.  tests/cpp/long_plan_check.cpp, a program of
its own built against the header alone with the address and undefined-behaviour sanitizers, runs all of them.  No library, no
Python extension and no GPU are involved."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_check(tmp_path, sanitize=True):
    exe = tmp_path / "long_plan_check"
    flags = ["-fsanitize=address,undefined"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-I",
                           os.path.join(ROOT, "recommendersystems_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "long_plan_check.cpp"), "-o", str(exe)])
    return exe


def test_long_plan(tmp_path):
    exe = build_check(tmp_path)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("0 failures"), r.stdout
