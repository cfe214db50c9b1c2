#!/usr/bin/env python3
"""GAPS and MIN_RHO of tests/graph_cases.py: for every case of the table and every iteration count k up to the case's, the
largest absolute difference of any pose entry and the relative differences of lambda and chi2_final between
graph_ref.optimize(solver="direct") and graph_ref.optimize(solver="pcg") (CPU only), the accept/reject pattern of the full
run under both solvers, the smallest |rho| of any trial and the smallest ratio |rho| / |rho_direct - rho_pcg|.
tests/test_gpu_graph.py allows the device 10 * GAPS against the direct solve. The two cases without a margin on rho (rho is
0, and NaN, by construction) have no gap: they are compared exactly. Usage: tools/graph_gap.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import graph_cases as GC   # noqa: E402


def main():
    rhos = {}
    print("GAPS = {    # case: per k = 1.., (pose, lambda, chi2_final)")
    for c in GC.CASES:
        _Pd, rd = GC.reference(c.name, c.iterations, "direct")
        _Pp, rp = GC.reference(c.name, c.iterations, "pcg")
        d, p = np.array([t["rho"] for t in rd["trace"]]), np.array([t["rho"] for t in rp["trace"]])
        note = "%s direct %s pcg %s" % (c.name, GC.pattern(rd), GC.pattern(rp))
        if c.name in GC.EXEMPT:
            print("    # %s, rho %s: exact comparison, no gap" % (note, sorted(set(map(str, p)))))
            continue
        rhos[c.name] = (min(np.abs(d).min(), np.abs(p).min()),
                        (np.minimum(np.abs(d), np.abs(p)) / np.maximum(np.abs(d - p), 1e-300)).min())
        print("    # %s" % note)
        print("    #   accepted rho %s" % " ".join("%.3f" % t["rho"] for t in rp["trace"] if t["accepted"]))
        rows = ["(%.2e, %.2e, %.2e)" % GC.gap(c.name, k) for k in range(1, c.iterations + 1)]
        lines = [", ".join(rows[k:k + 3]) for k in range(0, len(rows), 3)]
        pad = " " * (9 + len(c.name))
        print('    "%s": [%s],' % (c.name, (",\n" + pad).join(lines)), flush=True)
    print("}")
    print("MIN_RHO = {    # case: smallest |rho| of any trial    (smallest |rho| / |rho_direct - rho_pcg|)")
    for name, (lo, margin) in rhos.items():
        print('    "%s": %.3f,    # %.3g' % (name, lo, margin))
    print("}")


if __name__ == "__main__":
    main()
