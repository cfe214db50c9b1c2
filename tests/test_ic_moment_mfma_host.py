"""The matrix-core moment phase of the batch k_describe, replayed on the host (tests/cpp/ic_moment_selftest.cpp).

The program includes the weight table the kernel uses (aria_slam_amd/csrc/ic_moment_weights.h) and restates the phase in plain
C++: the lane -> operand maps, the piece order, the byte XOR, the int8 products and the result map, for random, all-0, all-255,
half-plane and random 0 / 255 windows at every x mod 16, and compares with the direct ICAngles loops of orb.cpp. It is built
with the address and undefined-behaviour sanitizers: a window piece that left its image would be a heap overflow."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "ic_moment_selftest.cpp")
HDR = os.path.join(ROOT, "aria_slam_amd", "csrc", "ic_moment_weights.h")


@pytest.fixture(scope="module")
def selftest():
    out_dir = os.path.join(ROOT, "build", "selftest")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "ic_moment_selftest")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I" + os.path.dirname(HDR), SRC, "-o", exe])
    return exe


def test_mfma_moments_equal_the_direct_loops(selftest):
    out = subprocess.run([selftest], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("OK ") and int(out.stdout.split()[1]) > 10000, out.stdout
