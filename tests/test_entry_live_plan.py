"""CPU-side check of the plan's per-link tile mask rule (recommendersystems_amd/csrc/step_plan.h): a step of
recommend_batch reads the masks (StepPlan::entry_live) only where it probes the frontier bitmaps and walks every row, at 8 or
more seeds per tile, in a group that has bitmaps and whose graph passes the size rule (RWR_ENTRY_LIVE=2: any size, 0: never);
never on a frontier-list or tail-list step, and never once the group's masks got no memory.
tests/cpp/entry_live_plan_check.cpp, built against the header alone with the address and undefined-behaviour sanitizers,
sweeps T <= 12, every tail depth and need mask, nz_iters 0-4, act_iters 0-3, lists on and off, every tile width and the three
settings of the knob.  No library and no GPU are needed."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_live_plan(tmp_path):
    exe = tmp_path / "entry_live_plan_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-I",
                           os.path.join(ROOT, "recommendersystems_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "entry_live_plan_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("0 failures"), r.stdout
