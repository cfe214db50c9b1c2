#!/usr/bin/env python3
"""GAP of tests/test_gpu_fuse.py and of tests/fuse_cases.py: the largest difference between the fp64 run and the
np.longdouble run of aria_slam_amd/fusion_ref.py on every test track and case (CPU only). States absolute; P and the
preintegration covariance relative to their largest entry. The tests allow the device 10 * GAP against the extended run
(fuse_cases.allowed puts scene1's row under a case that measures less). Usage: tools/fuse_gap.py"""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
spec = importlib.util.spec_from_file_location("test_gpu_fuse", os.path.join(ROOT, "tests", "test_gpu_fuse.py"))
T = importlib.util.module_from_spec(spec)
spec.loader.exec_module(T)
import fuse_cases as FC   # noqa: E402


def main():
    from aria_slam_amd import fusion_ref as R
    print("    track      states     P (rel)")
    for name in T.TRACKS:
        s64, f64, sld, fld = T.ref_runs(name)
        gs = max(float(np.abs(s64[k] - sld[k]).max()) for k in T.STATE_KEYS)
        gs = max(gs, max(float(np.abs(getattr(f64, a) - getattr(fld, a)).max())
                         for a in ("position", "velocity", "orientation", "accel_bias", "gyro_bias")))
        gp = float(np.abs(f64.P - fld.P).max() / np.abs(fld.P).max())
        gd = float(np.abs(s64["P_diag"] - sld["P_diag"]).max() / np.abs(sld["P_diag"]).max())
        for k in T.COUNTERS:
            assert np.array_equal(s64[k], sld[k]), (name, k)
        print("    %-9s  %.2e   %.2e" % (name, gs, max(gp, gd)), flush=True)
    imu, begin, end, bias = T.make_intervals()
    a = R.preintegrate(imu, begin, end, bias)
    b = R.preintegrate(imu, begin, end, bias, dtype=np.longdouble)
    gs = max(float(np.abs(a[k] - b[k]).max()) for k in ("delta_p", "delta_v", "delta_q", "dt_sum"))
    gc = float(np.abs(a["cov"] - b["cov"]).max() / np.abs(b["cov"]).max())
    print("    preint     %.2e   %.2e" % (gs, gc))
    print("the cases of tests/fuse_cases.py (GAP, as a dict's rows)")
    for name in FC.NAMES:
        print('    "%s": (%.2e, %.2e),' % ((name,) + FC.measure_gap(name)), flush=True)
    print("its interval kinds (PREINT_GAP)")
    for kind in FC.PREINT_KINDS:
        print('    "%s": (%.2e, %.2e),' % ((kind,) + FC.measure_preint_gap(kind)), flush=True)


if __name__ == "__main__":
    main()
