"""CPU-side check of the explained entry's host plan (recommendersystems_amd/csrc/explain_plan.h): the addend as two separately
rounded products, the selection model the reasons kernel compiles -- best n_why by (value bits descending, in-list position
ascending) and why_total -- against a brute-force sort for n_why = 0..8, in-degrees 0, 1, n_why - 1 .. n_why + 1, 63, 64, 65, 255 ..
257, 513 and 700, lane counts 1, 2, 64 and 256, with ties everywhere and with mostly zero sources, and the table sizes and
offsets.  (The verdicts on the arguments of rwr_recommend_explained_batch are tests/test_typed_call.py's.)
tests/cpp/explain_plan_check.cpp, a program of its own built against the header alone with the address and undefined-behaviour
sanitizers, compares all of them with brute-force loops.  No library, no Python extension and no GPU are involved."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_explain_plan(tmp_path):
    exe = tmp_path / "explain_plan_check"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-I",
                           os.path.join(ROOT, "recommendersystems_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "explain_plan_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("0 failures"), r.stdout
