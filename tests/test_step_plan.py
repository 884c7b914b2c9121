"""CPU-side check of the step plan (recommendersystems_amd/csrc/step_plan.h): what each power-iteration step of a tile group
does -- the rows its SpMM walks, the frontier bitmaps it reads and writes, the seed-row chain beside it, whether it forms the
next z.  tests/cpp/step_plan_check.cpp, built against the header alone, pins the plans of C4's group and of its variants
(RWR_TAIL_ROWS=0, RWR_TAIL_DEPTH=2, RWR_FRONTIER_LIST=0, RWR_ACT_ITERS=0, a single seed, a model batch, a threshold run) and
checks DESIGN §3.3.1 / §3.3.2's rules on every step of a sweep of groups.  No library and no GPU are needed."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_step_plan(tmp_path):
    exe = tmp_path / "step_plan_check"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I",
                           os.path.join(ROOT, "recommendersystems_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "step_plan_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("0 failures"), r.stdout
