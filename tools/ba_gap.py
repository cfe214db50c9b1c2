#!/usr/bin/env python3
"""The tolerance table of the bundle-adjustment tests, measured on the CPU with the restatement alone (no GPU, no library).

For every case of tests/ba_cases.py and every iteration count 1..K: the largest of (a) ba_ref(solver="schur") against
ba_ref(solver="full") and (b) ba_ref(solver="schur") against the same with every sum taken in reversed order, over every
pose entry, every point, lambda and chi2_final (each difference divided by max(1, |value|)). Also every case's
accept/reject pattern under the three runs, the smallest |rho| of any decision with its margin over the solvers'
difference, the smallest distance of a decision on depth from min_depth, and the restatement's errors against the
generator's truth before and after. The output is what tests/ba_cases.py holds as PATTERNS, GAPS, MIN_RHO and GT.

    python tools/ba_gap.py            # every case
    python tools/ba_gap.py --search   # the seed search the rejecting cases came from"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ba_cases as BC                         # noqa: E402
from aria_slam_amd import ba_ref as B         # noqa: E402


def letters(res):
    return "".join("A" if t["accepted"] else ("b" if t["solved"] and t["chi2_new"] == np.inf else "r") for t in res["trace"])


def search():
    sets = [dict(poses=5, points=40, pose_noise=0.1, point_noise=0.3, depth=(0.4, 2.0)),
            dict(poses=6, points=30, pose_noise=0.2, point_noise=0.4, depth=(0.5, 3.0), visibility=(2, 6))]
    for kw in sets:
        print(kw)
        for seed in range(40):
            win, _ = B.random_window(seed, **kw)
            with np.errstate(all="ignore"):
                _p, _x, r = B.optimize(win, BC.K_ITER)
            if "r" in letters(r) or "b" in letters(r):
                print("  seed %2d %s (r: by its gain, b: behind a camera)" % (seed, letters(r)))


def main():
    if "--search" in sys.argv:
        return search()
    pats, gaps, rhos, gts = [], [], [], []
    for c in BC.CASES:
        ref, full, rev = BC.reference(c.name), BC.reference(c.name, "full"), BC.reference(c.name, "schur", True)
        ps = [letters(r[2]) for r in (ref, full, rev)]
        pats.append('    "%s": "%s",%s' % (c.name, BC.pattern(ref[2]), "" if len(set(ps)) == 1 else "   # DIFFER: %s" % ps))
        if c.name not in BC.EXEMPT:
            gaps.append('    "%s": [%s],    # %s' % (c.name, ", ".join("%.2e" % BC.gap(c.name, k) for k in range(1, c.K + 1)), ps[0]))
            margin, zdist = BC.decision_margins(c.name)
            rhos.append('    "%s": %.3g,    # margin %.3g, depth decisions at least %.3g from min_depth' %
                        (c.name, min(abs(t["rho"]) for t in ref[2]["trace"] if np.isfinite(t["rho"])), margin, zdist))
        win, truth = BC.scene(c.name)
        if truth is not None:
            before, after = B.truth_errors(win["poses"], win["points"], truth, win), B.truth_errors(ref[0], ref[1], truth, win)
            gts.append('    "%s": ((%.4g, %.4g), (%.4g, %.4g)),' % ((c.name,) + before + after))
    print("PATTERNS = {\n%s\n}" % "\n".join(pats))
    print("GAPS = {    # case: per k = 1.., the largest scaled difference\n%s\n}" % "\n".join(gaps))
    print("MIN_RHO = {    # case: smallest |rho| of any decision\n%s\n}" % "\n".join(rhos))
    print("GT = {    # case: (mean pose, mean point error) before, after\n%s\n}" % "\n".join(gts))


if __name__ == "__main__":
    main()
