"""CPU-side check of the staging layout of ego-network-sized graphs (recommendersystems_amd/csrc/stage_layout.h): the six
raw arrays of the one upload copy are aligned, disjoint and end below the read-back area, the read-back area fits the pinned
buffer, its named offsets are the ones the build has always written, and the limits are the ones the one-launch paths test.
tests/cpp/stage_layout_check.cpp is built against the header alone, as a stand-alone program with the address and
undefined-behaviour sanitizers.  No library, no Python extension and no GPU are involved."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stage_layout(tmp_path):
    exe = tmp_path / "stage_layout_check"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "recommendersystems_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "stage_layout_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("0 failures"), r.stdout
