"""CPU-side check of the evaluation plan (recommendersystems_amd/csrc/eval_plan.h): what rwr_recommend_restart_eval_batch
puts on the device to evaluate its walks -- the test sets sorted and de-duplicated in slot order with one offset per slot and per
tile group, the buffer sizes, the exact layout of a tile group's hit lists and interval counters from its hit counts, and the
validation verdicts of the test sets.  tests/cpp/eval_plan_check.cpp, built against the header alone with the address and
undefined-behaviour sanitizers, compares them with a direct restatement.  No library, no Python extension and no GPU are
involved."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_eval_plan(tmp_path):
    exe = tmp_path / "eval_plan_check"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-I",
                           os.path.join(ROOT, "recommendersystems_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "eval_plan_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("0 failures"), r.stdout
