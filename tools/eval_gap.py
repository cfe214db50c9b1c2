#!/usr/bin/env python3
"""GAP table of trajectory evaluation (tests/test_gpu_eval.py): for every named track of
aria_slam_amd.eval_ref the largest difference between the restatement run in np.float64 and in np.longdouble. The device is
held to 10 x GAP against the extended run. CPU only."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aria_slam_amd import eval_ref as R   # noqa: E402

if __name__ == "__main__":
    print("%-10s %-5s %12s %12s %12s   %s" % ("track", "mode", "metres", "R, scale", "sigma (rel)", "sigma2/sigma1"))
    for name in R.TRACK_NAMES:
        for mode, label in ((R.ALIGN_SIM3, "sim3"), (R.ALIGN_SE3, "se3")):
            (m, r, s), hi = R.track_gap(name, mode)
            print("%-10s %-5s %12.2e %12.2e %12.2e   %.3e" % (name, label, m, r, s, float(hi["sigma"][1] / hi["sigma"][0])))
    g, _ = R.sampler_gap()
    print("%-10s %-5s %12.2e" % ("sampler", "-", g))
