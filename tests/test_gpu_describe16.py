"""k_describe's batch Q4 form (16 keypoints per wave) against the oracle byte for byte, at the shapes that exercise its
edges (tools/describe16_check.py: level counts of every residue mod 16, a kp_cap overflow, a tie-storm arena, the
1408x1408 / 4000-keypoint shape) -- in the product library, and in the variants build both with its default and with
the 4-keypoints-per-wave body it replaced (ARIA_DESC_IMPL=quad)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["levels", "kpcap", "tiestorm", "big"]


@pytest.fixture(scope="module")
def variants_lib():
    sys.path.insert(0, ROOT)
    import aria_slam_amd
    return aria_slam_amd.build_variants_library()


def _run(env, case):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "describe16_check.py"), case], env=env,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count("OK ") == 1, out.stdout


@pytest.mark.parametrize("case", CASES)
def test_describe16_product(aria, case):
    e = dict(os.environ)
    e.pop("ARIA_ORB_HIP_LIBRARY", None)
    _run(e, case)


@pytest.mark.parametrize("impl", ["default", "quad"])
@pytest.mark.parametrize("case", CASES)
def test_describe16_variants(variants_lib, case, impl):
    e = dict(os.environ)
    e["ARIA_ORB_HIP_LIBRARY"] = variants_lib
    if impl == "quad":
        e["ARIA_DESC_IMPL"] = "quad"
    _run(e, case)
