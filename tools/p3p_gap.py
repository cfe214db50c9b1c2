#!/usr/bin/env python3
"""GAP of tests/test_gpu_p3p.py: for every exact-set case of tests/p3p_cases.py, the largest difference of R, t and rms_px
between the fp64 run and the np.longdouble run of the restatement with the P3P solver (aria_slam_amd/pnp_ref.py, CPU only).
The tests compute the same figures from p3p_cases.gap and allow the device 10 * GAP against the extended run. Also the
restatement's error against ground truth over the planar cases, whose worst the device is allowed twice
(p3p_cases.PLANAR_TRUTH_ERROR).
Usage: tools/p3p_gap.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import p3p_cases as QC   # noqa: E402


def main():
    for name, cases in (("P3P_CASES", QC.P3P_CASES), ("P3P_BATCH", QC.P3P_BATCH)):
        print("%s: case  n  H  valid  winner  slot  in-band  GAP R  t  rms_px" % name)
        for i, c in enumerate(cases):
            rep = QC.report(c)
            ref = rep["ref"]
            if not ref["valid"]:
                print("    %2d  %4d  %4d  0    # %s" % (i, c.n, c.H, QC.case_id(c)))
                continue
            gap = QC.gap(c) if rep["exact"] else (float("nan"),) * 3
            print("    %2d  %4d  %4d  1  %4d  %d  %d  %.2e  %.2e  %.2e    # %s" %
                  ((i, c.n, c.H, ref["best_hypothesis"], rep["slots"][ref["best_hypothesis"]], rep["in_band"]) + gap + (QC.case_id(c),)),
                  flush=True)
    worst = [0.0, 0.0, 1.0]
    for i in QC.PLANAR_CASES:
        rep = QC.report(QC.P3P_CASES[i])
        r, t, prec = QC.truth_error(rep["ref"], rep)
        print("ground truth, planar case %2d: rotation %.4f deg, |t - t_true| %.5f, mask precision %.4f" % (i, r, t, prec))
        worst = [max(worst[0], r), max(worst[1], t), min(worst[2], prec)]
    print("PLANAR_TRUTH_ERROR = (%.5f, %.6f)    # rotation (deg), translation; mask precision %.4f" % tuple(worst))


if __name__ == "__main__":
    main()
