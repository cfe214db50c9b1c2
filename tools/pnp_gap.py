#!/usr/bin/env python3
"""GAP of tests/test_gpu_pnp.py: for every exact-set case of tests/pnp_cases.py, the largest difference of R, t and rms_px
between the fp64 run and the np.longdouble run of the restatement (aria_slam_amd/pnp_ref.py, CPU only), whose refinement,
nearest rotation and outputs run in extended precision. The tests allow the device 10 * GAP against the extended run.
Also the restatement's worst error against ground truth over pnp_cases.GT_CASES, which the device is allowed twice.
Usage: tools/pnp_gap.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pnp_cases as PC   # noqa: E402


def main():
    for name, cases in (("PNP_GAP", PC.PNP_CASES), ("PNP_BATCH_GAP", PC.PNP_BATCH)):
        print("%s = {    # case: (R, t, rms_px)" % name)
        for i, c in enumerate(cases):
            rep = PC.report(c)
            if rep["exact"] and rep["ref"]["valid"]:
                print("    %2d: (%.2e, %.2e, %.2e),    # %s" % ((i,) + PC.gap(c) + (PC.case_id(c),)), flush=True)
        print("}")
    worst = [0.0, 0.0, 1.0]
    for i in PC.GT_CASES:
        rep = PC.report(PC.PNP_CASES[i])
        r, t, prec = PC.truth_error(rep["ref"], rep)
        print("ground truth, case %2d: rotation %.4f deg, |t - t_true| %.5f, mask precision %.4f" % (i, r, t, prec))
        worst = [max(worst[0], r), max(worst[1], t), min(worst[2], prec)]
    print("GT_WORST = (%.4f, %.5f, %.4f)    # rotation (deg), translation, mask precision" % tuple(worst))


if __name__ == "__main__":
    main()
