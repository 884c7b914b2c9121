"""CPU-side check of the seed-driven typed entries' one call description (recommendersystems_amd/csrc/typed_call.h): for each of
the eight entries -- rwr_recommend_typed_batch, _typed_eval_batch, _typed_positions_batch, _filtered_batch,
_filtered_positions_batch, _capped_batch, _capped_positions_batch and _explained_batch -- the flat verdict and the first-offender
positions of every single finding, of every finding beside all later ones (every fault present, peeled off one at a time: the
entry's documented order of refusals), random combinations against a restatement of the header comments, the check the two typed
restart-vector entries add, and the status and the whole message of every refusal of every entry against literals.
tests/cpp/typed_call_check.cpp, a program of its own built against the headers alone with the address and undefined-behaviour
sanitizers, holds all of it.  No library, no Python extension and no GPU are involved."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_typed_call(tmp_path):
    exe = tmp_path / "typed_call_check"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-I",
                           os.path.join(ROOT, "recommendersystems_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "typed_call_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("0 failures"), r.stdout
