#!/usr/bin/env python3
"""GAP of tests/test_gpu_map.py and tests/test_gpu_map_scale.py: for every scene on which the device's point records are
compared with aria_slam_amd/map_ref.py (tests/map_cases.py lists them), the largest difference between the restatement's
fp64 run and its np.longdouble run over the points both keep (CPU only): X relative, err absolute (pixels), quality
relative. The tests allow the device 10 * GAP on X and quality against the extended run. Also the smallest relative
distance of any tested quantity of the extended run to its threshold, which tests/test_map_host.py holds above 1e-9 so that
the kept set is compared without a margin. Usage: tools/map_gap.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import map_cases   # noqa: E402


def main():
    print("    scene    X (rel)    err (abs)  quality (rel)  margin    kept")
    for name in map_cases.SCENES:
        a, b = map_cases.ref_runs(name)
        assert (a["keep"] == b["keep"]).all(), name
        gx, ge, gq, margin = map_cases.gap(name)
        print("    %-7s  %.2e   %.2e   %.2e       %.1e   %d of %d" % (name, gx, ge, gq, margin, b["keep"].sum(), len(b["keep"])),
              flush=True)


if __name__ == "__main__":
    main()
