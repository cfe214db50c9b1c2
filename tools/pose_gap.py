#!/usr/bin/env python3
"""GAP of tests/test_gpu_pose.py and tests/test_gpu_fund.py: for every exact-set case of tests/ransac_cases.py, the largest
difference between the fp64 run and the np.longdouble run of the restatement (CPU only). Pose: E (unit norm, sign-aligned),
R and t of aria_slam_amd/pose_ref.py's estimate, whose refit, decomposition and depths run through jacobi_eigh in the
extended run. Fundamental: the winning model of fund_ref.solve7, scaled by its largest entry. The tests allow the device
10 * GAP against the extended run. Usage: tools/pose_gap.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ransac_cases as RC   # noqa: E402


def main():
    for name, cases in (("POSE_GAP", RC.POSE_CASES), ("POSE_BATCH_GAP", RC.POSE_BATCH)):
        print("%s = {    # case: (E, R, t)" % name)
        for i, c in enumerate(cases):
            rep = RC.pose_report(c)
            if rep["exact"] and rep["ref"]["valid"]:
                print("    %2d: (%.2e, %.2e, %.2e),    # %s" % ((i,) + RC.pose_gap(c) + (RC.case_id(c),)), flush=True)
        print("}")
    for name, cases in (("FUND_GAP", RC.FUND_CASES), ("FUND_BATCH_GAP", RC.FUND_BATCH)):
        print("%s = {    # case: F" % name)
        for i, c in enumerate(cases):
            rep = RC.fund_report(c)
            if rep["exact"] and rep["ref"]["valid"]:
                print("    %2d: %.2e,    # %s" % (i, RC.fund_gap(c), RC.case_id(c)), flush=True)
        print("}")


if __name__ == "__main__":
    main()
