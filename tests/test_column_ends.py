"""CPU-side check of the column ends of a tile group of Models (recommendersystems_amd/csrc/column_ends.h): which columns
of rwr_model_run_batch / rwr_model_run_restart_batch leave after which step -- every real one after step T in iteration
mode, each after the first step at which its own distance is below the threshold otherwise -- their staging rows, their
iteration counts and the column that RWR_MAX_ITERS names.  tests/cpp/column_ends_check.cpp, built against the header alone
with the address and undefined-behaviour sanitizers, compares it with a per-column simulation over scripted distances.
No library, no Python extension and no GPU are involved."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_column_ends(tmp_path):
    exe = tmp_path / "column_ends_check"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-I",
                           os.path.join(ROOT, "recommendersystems_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "column_ends_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("0 failures"), r.stdout
