"""CPU-side check of the device-memory block cache behind every DevBuf (recommendersystems_amd/csrc/pool.h): the size
classes, the per-thread cache in front of the per-device shared one, their three caps, the out-of-memory retry and what a
thread leaves behind when it ends.  tests/cpp/pool_check.cpp, built against the header alone, drives it with a raw allocator
of tokens: once with the address and undefined-behaviour sanitizers, once with the thread sanitizer (ten threads, the
harness's count).  No library, no Python extension and no GPU are involved."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ADDR_NO_RANDOMIZE = 0x0040000


def _fixed_address_space():
    """The check runs without address-space randomisation (for this child process alone): the thread sanitizer's runtime of
    older compilers gives up with "unexpected memory mapping" where the kernel randomises 32 bits of a mapping's address."""
    libc = ctypes.CDLL(None)
    libc.personality(libc.personality(0xFFFFFFFF) | ADDR_NO_RANDOMIZE)


@pytest.mark.parametrize("sanitizers", ["address,undefined", "thread"])
def test_pool(tmp_path, sanitizers):
    exe = tmp_path / "pool_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-pthread", "-fsanitize=" + sanitizers,
                           "-I", os.path.join(ROOT, "recommendersystems_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "pool_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, preexec_fn=_fixed_address_space)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("0 failures"), r.stdout
    assert "Sanitizer" not in r.stderr, r.stderr
