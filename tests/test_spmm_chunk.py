"""CPU-side check of how the chunked SpMM cuts a row's in-list into index loads (recommendersystems_amd/csrc/spmm_chunk.h,
DESIGN §3.3): tests/cpp/spmm_chunk_check.cpp, built against the header alone with the address and undefined-behaviour
sanitizers, walks every list start 0..95, every length 0..200 and the load widths 8, 16 and 32.  No library and no GPU are
needed."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_spmm_chunk(tmp_path):
    exe = tmp_path / "spmm_chunk_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "recommendersystems_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "spmm_chunk_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("0 failures"), r.stdout
    assert r.stdout.strip().startswith(str(3 * 96 * 201) + " combinations"), r.stdout
