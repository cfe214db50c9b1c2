#!/usr/bin/env python3
"""The two exact selections of the obstacle-alert stage on the measurement cases of tests/alert_cases.py: the shipped radix
selection and the 32-pass bitwise bisection of the variants build (ARIA_ALERT_SELECT=plain, read when a handle is created) give
the same records, bit for bit, and both equal the restatement. ARIA_ORB_HIP_LIBRARY must name the variants build: the product
library knows no switch and would run the shipped kernel twice, so anything else is refused. Prints one line per case and "alert selections agree"."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import torch
    import aria_slam_amd as A
    import alert_cases as AC
    from aria_slam_amd import alert_ref as R
    assert A.library_path().endswith("libaria_orb_hip_variants.so"), "set ARIA_ORB_HIP_LIBRARY to the variants build"
    assert torch.cuda.is_available()
    for (W, H), pad, pct in (((37, 19), 5, "default"), ((64, 24), 0, "first"), ((300, 200), 5, "default"), ((300, 200), 0, "last")):
        case = AC.measure_case(W, H, pad, pct)
        got = {}
        for name in ("radix", "plain"):
            if name == "plain":
                os.environ["ARIA_ALERT_SELECT"] = "plain"
            h = A.HipObstacleAlerter.from_ref_config(case.cfg)
            os.environ.pop("ARIA_ALERT_SELECT", None)
            got[name], status = h.measure(case.depth, case.dets, case.ndets)
            assert status == R.E_INVALID == case.status      # the case's counts outside [0, det_cap]
            h.close()
        for name, m in got.items():
            print("%dx%d pad %d %s %s: %d of %d records differ from the restatement" % (W, H, pad, pct, name, int((m != case.meas).sum()), m.size))
            assert m.tobytes() == case.meas.tobytes(), name
        assert np.isfinite(got["plain"]["distance"]).all()
    print("alert selections agree")


if __name__ == "__main__":
    main()
