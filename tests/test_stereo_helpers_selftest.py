"""The pure helpers of aria_slam_amd/csrc/stereo_match.hip on the host (tests/cpp/stereo_helpers_selftest.cpp).

The text of ld_u32, load_row<HW>, sad_slide<HW>, hist_select, order_key and key_value is cut out of the .hip file between its
marker comments, with the ST_* constants above them, and compiled for the host with a one-line stand-in for the SAD instruction.
The program holds load_row and sad_slide to a plain byte loop for every window 1..7, every slide of 3..33 shifts and every lane,
hist_select to a sorted list, and the key pair to std::sort on doubles of both signs, zeros, denormals and infinities. It is a
stand-alone program built with the address and undefined-behaviour sanitizers, and every row it hands over starts and ends with
its heap block: a read outside the row is a heap overflow.

What this cannot check: the shuffles, the LDS and its atomics, the barriers. That is tests/test_gpu_stereo_edges.py."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "stereo_helpers_selftest.cpp")
HIP = os.path.join(ROOT, "aria_slam_amd", "csrc", "stereo_match.hip")
MARKS = (("// ---- pure helpers: plain C++ of one lane", "// ---- end of the pure helpers ----"),
         ("// ---- pure helpers of the scale ----", "// ---- end of the pure helpers of the scale ----"))


@pytest.fixture(scope="module")
def selftest():
    src = open(HIP).read()
    consts = re.findall(r"^constexpr int ST_[^\n]*$", src, re.M)
    assert len(consts) == 9
    pasted = "\n".join(consts) + "\n" + "\n".join(src[src.index(a):src.index(b)] for a, b in MARKS)
    for fn in ("ld_u32", "load_row", "sad_slide", "hist_select", "order_key", "key_value"):
        assert re.search(r"\b%s\(" % fn, pasted), fn
    for word in ("__shared__", "__syncthreads", "__shfl", "__ballot", "atomic", "asm", "__global__"):
        assert word not in pasted, "plain C++ of one lane: no LDS, no barrier, no cross-lane operation (%s)" % word
    out_dir = os.path.join(ROOT, "build", "selftest", "stereo_helpers")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "stereo_helpers_pasted.inc"), "w") as f:
        f.write(pasted)
    exe = os.path.join(out_dir, "stereo_helpers_selftest")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + out_dir, SRC, "-o", exe])
    return exe


def test_helpers_equal_the_plain_loops_and_stay_inside_their_rows(selftest):
    out = subprocess.run([selftest], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("OK ") and int(out.stdout.split()[1]) > 20000, out.stdout
