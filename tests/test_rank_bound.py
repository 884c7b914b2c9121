"""CPU-side check of the rounding behind the pruned body of a batch's last step (recommendersystems_amd/csrc/rank_bound.h,
DESIGN §3.3.3): tests/cpp/rank_bound_check.cpp, built against the header alone, sums random non-negative doubles in list order
as k_spmm_select does and checks that the float bound never falls below that sum divided by the threshold -- a row that
reaches its threshold, ties included, is never pruned.  No library and no GPU are needed."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rank_bound(tmp_path):
    exe = tmp_path / "rank_bound_check"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I",
                           os.path.join(ROOT, "recommendersystems_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "rank_bound_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("0 failures"), r.stdout
