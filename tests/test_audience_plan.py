"""CPU-side check of the audience entry's host plan (recommendersystems_amd/csrc/audience_plan.h): the ladder of refusals in its
documented order (every later fault present, the earlier one wins; the no-op last), the long-row split of the reverse step at
out-degrees 0, 1, 4, 5, split - 1, split, split + 1 and several pieces, the target-to-column table with repeated targets, padding
slots and several tile groups, the two device-side searches, the workspace sizes in 64-bit arithmetic, and the restart-mass
recurrence against the formula written out.  tests/cpp/audience_plan_check.cpp, a program of its own built against the header
alone with the address and undefined-behaviour sanitizers, compares all of them with brute-force loops.  No library, no Python
extension and no GPU are involved."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_check(tmp_path, sanitize=True):
    exe = tmp_path / "audience_plan_check"
    flags = ["-fsanitize=address,undefined"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-I",
                           os.path.join(ROOT, "recommendersystems_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "audience_plan_check.cpp"), "-o", str(exe)])
    return exe


def test_audience_plan(tmp_path):
    exe = build_check(tmp_path)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("0 failures"), r.stdout
