"""The yardstick selection of the obstacle-alert stage (k_alert_measure_plain, variants build only) against the shipped radix
selection and the restatement, so that the kernel tools/alert_rate.py times against stays correct. As tests/test_gpu_variants.py
does, this module builds libaria_orb_hip_variants.so itself and points a subprocess's binding at it."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bisection_equals_the_radix_selection_and_the_restatement(aria):
    e = dict(os.environ)
    e["ARIA_ORB_HIP_LIBRARY"] = aria.build_variants_library()
    e.pop("ARIA_ALERT_SELECT", None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "alert_select_check.py")], env=e, capture_output=True, text=True,
                         timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count("plain: 0 of") == 4 and out.stdout.count("radix: 0 of") == 4 and "alert selections agree" in out.stdout
