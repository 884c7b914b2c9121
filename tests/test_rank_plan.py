"""CPU-side check of the ranking stage's host-side decisions (recommendersystems_amd/csrc/rank_plan.h):
tests/cpp/rank_plan_check.cpp, built against the header alone, pins the defaults of the environment values, the head size of a
batch's last step at the size threshold, on both matrix paths and at the powers of two, and the candidate capacity per seed.
No library and no GPU are needed."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rank_plan(tmp_path):
    exe = tmp_path / "rank_plan_check"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I",
                           os.path.join(ROOT, "recommendersystems_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "rank_plan_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("0 failures"), r.stdout
