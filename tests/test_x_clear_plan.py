"""CPU-side check of the plan's X-clear decision (recommendersystems_amd/csrc/step_plan.h): a ranking-only batch
on the frontier-list path does not clear its rank matrix, so the fold that reads every row of the list step's output must read
it through that step's bitmap (StepPlan::chain_masked), and a group whose chain has no masked form -- the binade scan, the
simple fold -- or that never lists keeps the clear (PlanConfig::clear_x).  tests/cpp/x_clear_plan_check.cpp, built against
the header alone with the address and undefined-behaviour sanitizers, sweeps T <= 12, every tail depth and need mask, lists on
and off, every chain kind, RWR_ACT_ITERS 1 and 2 and RWR_X_CLEAR=1.  No library and no GPU are needed."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_x_clear_plan(tmp_path):
    exe = tmp_path / "x_clear_plan_check"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-I",
                           os.path.join(ROOT, "recommendersystems_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "x_clear_plan_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("0 failures"), r.stdout
