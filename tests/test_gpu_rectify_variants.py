"""The rejected read form of the rectification stage (k_rect_remap_lds, variants build only) and the ARIA_RECT_READ /
ARIA_RECT_GROUP switches against the restatement, so that the kernels tools/rect_rate.py times against, and the numbers of
DESIGN.md section 19 that rest on them, stay held to the definition. As tests/test_gpu_alert_variants.py does, this module
builds libaria_orb_hip_variants.so itself and points a subprocess's binding at it; tools/rect_check.py runs every remap case
of tests/rectify_cases.py, zoom20_big (tiles that do and do not fit the LDS) included."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rectify_cases as RC   # noqa: E402


@pytest.fixture(scope="module")
def variants_library(aria):
    return aria.build_variants_library()


@pytest.mark.parametrize("setting", RC.VARIANT_SETTINGS, ids=lambda s: ",".join("%s=%s" % kv for kv in s.items()) or "shipped")
def test_every_read_form_and_frame_group_equals_the_restatement(variants_library, setting):
    e = dict(os.environ)
    e["ARIA_ORB_HIP_LIBRARY"] = variants_library
    for k in ("ARIA_RECT_READ", "ARIA_RECT_GROUP"):
        e.pop(k, None)
    e.update(setting)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "rect_check.py")], env=e, capture_output=True, text=True,
                         timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "library libaria_orb_hip_variants.so" in out.stdout
    for name, case in RC.EDGE_CASES.items():
        assert "%s: 0 of %d pixels differ\n" % (name, case.want.size) in out.stdout, name
    assert out.stdout.count(" pixels differ") == len(RC.EDGE_CASES) == 9
