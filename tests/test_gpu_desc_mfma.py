"""The batch k_describe's matrix-core moment phase against the oracle byte for byte (tools/desc_moments_check.py: keypoint
records with their angles and descriptors of every keypoint) -- byte-unaligned level-0 rows, saturated windows of both
signs, keypoints on the border of the valid region -- and the build that keeps the LDS moment rounds for MODE 0
(-DARIA_DESC_MOMENTS_LDS=1, the A side of A/B measurements) on the first case."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aria_slam_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def checker(aria, oracle):
    assert not os.environ.get("ARIA_ORB_HIP_LIBRARY"), "these cases are about the product library"
    import desc_moments_check
    return desc_moments_check


@pytest.mark.parametrize("case", ["pair", "unaligned", "rects", "edges"])
def test_batch_moments_equal_the_oracle(checker, case):
    getattr(checker, "case_" + case)()


@pytest.fixture(scope="module")
def lds_lib():
    so = os.path.join(ROOT, "build", "ab", "libdesc_lds.so")
    newest = max(os.path.getmtime(os.path.join(CSRC, f)) for f in os.listdir(CSRC) if f.endswith((".hip", ".h", ".cpp", ".inc")))
    if not os.path.exists(so) or os.path.getmtime(so) < newest:
        subprocess.check_call(["bash", os.path.join(ROOT, "tools", "build_ab.sh"), "desc_lds", "-DARIA_DESC_MOMENTS_LDS=1"])
    return so


def test_lds_moment_build_equals_the_oracle(aria, oracle, lds_lib):
    e = dict(os.environ)
    e["ARIA_ORB_HIP_LIBRARY"] = lds_lib
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "desc_moments_check.py"), "pair"], env=e,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count("OK ") == 1, out.stdout
