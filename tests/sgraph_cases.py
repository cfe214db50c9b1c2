"""The case table of the Sim(3) pose-graph stage, shared by the CPU test (tests/test_sgraph_host.py), the GPU test
(tests/test_gpu_sgraph.py: the device against sgraph_ref at every iteration count up to the case's) and tools/sgraph_gap.py
(the tolerance tables). A plain module: no fixtures, no pytest. The method and the format are those of tests/graph_cases.py.

A case is Case(name, args, fixed, iterations, fix_scale, pattern, handle, note). The graph is sgraph_ref.random_sgraph(*args),
args = (seed, n_vertices, n_extra_edges, noise): vertex scales in [0.5, 2]; with fix_scale every vertex and edge scale is 1
(the metric map the flag is for). `pattern` is one letter per trial of sgraph_ref.optimize(..., iterations), A accepted and r
rejected. `handle` is (max_vertices, max_edges) of the optimiser the GPU test creates for the case; None takes the module's
shared one (512, 1024).

One form of the solve is built (every lane owns the vertices lane + k * 512), so the boundary cases are one more vertex than a
lane per vertex holds ("v513": a lane's second vertex) and one more edge than a lane per edge holds ("e513": a lane's second
edge in the linearising pass, at 200 vertices).

LIN_GRAPHS are the graphs of the debug_linearize test: (name, args, fixed). "tiny" is 3 vertices and 2 edges with the middle
vertex fixed, so both others hang on the fixed one alone.

LIN_GAPS[name] = (chi2, b, H_diag, H_off): the difference between sgraph_ref.linearize in fp64 and the same formulas in
numpy.longdouble (tools/sgraph_gap.py), chi2 relative, each array as max |difference| / max |entry|. The device is allowed
ten times each.
GAPS[name][k - 1] = (vertex, lambda, chi2_final): after k iterations, the largest absolute difference of any vertex entry and
the relative differences of lambda and chi2_final between sgraph_ref.optimize(solver="direct") and (solver="pcg"), measured
on the CPU. The device is allowed ten times each against the direct solve. MIN_RHO[name] is the smallest |rho| of any trial.
FIX_SCALE_GAP is the largest pose difference between sgraph_ref.optimize(fix_scale) and graph_ref.optimize on the SE(3) graph
"se3" (every scale 1) under the pcg solver, from the same tool; tests/test_sgraph_host.py allows ten times it.
All copied from the output of tools/sgraph_gap.py."""
import collections
import functools

import numpy as np

from aria_slam_amd import graph_ref as G
from aria_slam_amd import sgraph_ref as S

Case = collections.namedtuple("Case", "name args fixed iterations fix_scale pattern handle note")

RHO_MIN = 1e-2             # every decision's |rho| is at least this ...
RHO_MARGIN = 1000.0        # ... and this many times the direct-vs-pcg difference of that trial's rho

CASES = [
    Case("random40", (31, 40, 12, 1.0), 0, 3, False, "AAA", None, "one random graph of 40 vertices"),
    Case("rejected", (31, 40, 12, 2.0), 0, 3, False, "rrrAAA", None, "three rejected trials before the first accept"),
    Case("fixed7", (34, 30, 8, 3.0), 7, 3, False, "rrrrAAA", None, "vertex 7 fixed"),
    Case("fixscale", (31, 40, 12, 2.0), 0, 3, True, "rrrAAA", None, "fix_scale on a graph whose scales are all 1"),
    Case("v513", (42, 513, 60, 3.0), 0, 2, False, "rrrrAA", (513, 1024), "513 vertices: a lane's second vertex"),
    Case("e513", (47, 200, 314, 3.0), 0, 2, False, "rrrAA", (256, 513), "513 edges: a lane's second edge"),
]
BY_NAME = {c.name: c for c in CASES}

LIN_GRAPHS = [("tiny", (5, 3, 0, 0.3), 1), ("v40e51", (6, 40, 12, 0.3), 0), ("v200e229", (7, 200, 30, 0.3), 3)]
SE3_GRAPH = (3, 12, 5)       # graph_ref.random_graph(*SE3_GRAPH): the graph of the fix_scale-against-graph_ref test
SE3_ITERATIONS = 5

# ---- the output of tools/sgraph_gap.py, copied
LIN_GAPS = {    # graph: (chi2, b, H_diag, H_off), fp64 against long double
    "tiny": (2.91e-16, 5.05e-16, 1.61e-16, 1.79e-16),    # 3 vertices, 2 edges
    "v40e51": (9.49e-17, 1.27e-15, 3.87e-16, 2.21e-16),    # 40 vertices, 51 edges
    "v200e229": (1.96e-16, 1.02e-15, 2.18e-16, 2.23e-16),    # 200 vertices, 229 edges
}
GAPS = {    # case: per k = 1.., (vertex, lambda, chi2_final)
    # random40 direct AAA pcg AAA
    #   accepted rho 0.411 0.898 0.896
    "random40": [(4.07e-06, 7.52e-08, 6.52e-07), (5.44e-06, 8.29e-07, 3.51e-07), (3.91e-06, 9.52e-07, 1.50e-07)],
    # rejected direct rrrAAA pcg rrrAAA
    #   accepted rho 0.418 0.055 0.524
    "rejected": [(4.44e-07, 2.59e-10, 2.70e-09), (6.37e-07, 2.36e-08, 5.63e-09), (8.63e-07, 2.32e-08, 4.17e-08)],
    # fixed7 direct rrrrAAA pcg rrrrAAA
    #   accepted rho 0.295 0.706 0.078
    "fixed7": [(1.71e-08, 8.59e-10, 9.00e-10), (6.22e-08, 4.70e-10, 1.33e-10), (5.11e-08, 1.19e-08, 3.01e-09)],
    # fixscale direct rrrAAA pcg rrrAAA
    #   accepted rho 0.440 0.250 0.405
    "fixscale": [(2.69e-07, 4.23e-10, 8.09e-09), (5.10e-07, 5.47e-08, 5.85e-08), (6.22e-07, 5.75e-08, 7.80e-08)],
    # v513 direct rrrrAA pcg rrrrAA
    #   accepted rho 0.696 0.746
    "v513": [(7.22e-08, 4.19e-10, 6.68e-10), (1.15e-07, 2.63e-10, 2.39e-11)],
    # e513 direct rrrAA pcg rrrAA
    #   accepted rho 0.241 0.592
    "e513": [(2.77e-07, 1.02e-08, 6.03e-09), (4.46e-07, 9.28e-09, 4.69e-10)],
}
MIN_RHO = {    # case: smallest |rho| of any trial    (smallest |rho| / |rho_direct - rho_pcg|)
    "random40": 0.411,    # 1.03e+06
    "rejected": 0.055,    # 2.57e+06
    "fixed7": 0.078,    # 7.07e+05
    "fixscale": 0.102,    # 7.2e+05
    "v513": 0.026,    # 7.8e+06
    "e513": 0.241,    # 4.24e+06
}
FIX_SCALE_GAP = 1.10e-10    # largest pose entry difference, sgraph_ref fix_scale against graph_ref


@functools.lru_cache(maxsize=None)
def graph(name):
    """(vertices (V, 13), edges) of a case."""
    c = BY_NAME[name]
    if c.fix_scale:                                   # the metric map: every vertex and edge scale exactly 1
        return S.random_sgraph(*c.args, scale_range=(1.0, 1.0), scale_noise=0.0)
    return S.random_sgraph(*c.args)


@functools.lru_cache(maxsize=None)
def lin_graph(name):
    args, fixed = {n: (a, f) for n, a, f in LIN_GRAPHS}[name]
    V, E = S.random_sgraph(*args)
    return V, E, fixed


@functools.lru_cache(maxsize=None)
def reference(name, k, solver):
    """sgraph_ref.optimize of a case after k iterations: (vertices, result dict with its trace)."""
    c = BY_NAME[name]
    V, E = graph(name)
    return S.optimize(V, E, c.fixed, k, solver, fix_scale=c.fix_scale)


def pattern(res):
    return "".join("A" if t["accepted"] else "r" for t in res["trace"])


def rel(a, b):
    """|a - b| / |b|; 0 where both are equal."""
    return 0.0 if a == b else abs(a - b) / abs(b)


def gap(name, k):
    """(vertex, lambda, chi2_final) between the pcg and the direct run of the restatement after k iterations."""
    (Vd, rd), (Vp, rp) = reference(name, k, "direct"), reference(name, k, "pcg")
    return float(np.abs(Vp - Vd).max()), rel(rp["lambda_"], rd["lambda_"]), rel(rp["chi2_final"], rd["chi2_final"])


def se3_graph():
    """(poses, edges) of graph_ref and the same graph as Sim(3) vertices and edges with every scale 1."""
    poses, edges = G.random_graph(*SE3_GRAPH)
    return poses, edges, S.vertices_from_poses(poses), [e + (1.0,) for e in edges]
