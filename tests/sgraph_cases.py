"""The case table of the Sim(3) pose-graph stage, shared by the CPU test (tests/test_sgraph_host.py), the GPU tests
(tests/test_gpu_sgraph.py, tests/test_gpu_sgraph_paths.py: the device against sgraph_ref at every iteration count up to the
case's) and tools/sgraph_gap.py (the tolerance tables). A plain module: no fixtures, no pytest. The method and the format are
those of tests/graph_cases.py.

A case is Case(name, args, fixed, iterations, fix_scale, pattern, handle, note, kind, pcg_max_iters). The graph by kind:
  "random"    sgraph_ref.random_sgraph(*args), args = (seed, n_vertices, n_extra_edges, noise): vertex scales in [0.5, 2]; with
              fix_scale every vertex and edge scale is 1 (the metric map the flag is for)
  "scaled"    random_sgraph(*args) with its scales in [0.5, 2] whatever fix_scale says
  "exact"     args = (n,): identity rotations, centres (0.5 i, 0.25 i, 0), scales 2^(i % 3 - 1), every chain edge exactly
              consistent at info_scale 1 and one exactly consistent loop edge 0 -> n-1 at 10: chi2 = 0, b = 0, every trial is
              a zero step with rho == 0 exactly, which rho > 0 rejects
  "overflow"  args = (seed, n_vertices, n_extra_edges, noise, info_scale): random_sgraph with every info_scale replaced
              (tests/graph_cases.py's header says why chi2_initial is not finite here)
  "topology"  args = (seed, noise): topology_graph below -- a chain, a hub joined to TOPO_HUB_DEGREE vertices, a free vertex with
              no edge, one edge with info_scale 0.0, one pair joined twice in one direction and once in the other
`pattern` is one letter per trial of sgraph_ref.optimize(..., iterations), A accepted and r rejected. `handle` is
(max_vertices, max_edges) of the optimiser the GPU test creates for the case; None takes the module's shared one (512, 1024).
`pcg_max_iters` is the solver's cap, the handle's and the restatement's.

Every run of k iterations is the first k iterations of the run of K > k (LM's state is rebuilt from the vertices at each call),
so the device's prefix runs k = 1..K pin the number of rejections before every accept.

One form of the solve is built (every lane owns the vertices lane + k * 512), so the boundary cases are one more vertex than a
lane per vertex holds ("v513": a lane's second vertex) and one more edge than a lane per edge holds ("e513": a lane's second
edge in the linearising pass, at 200 vertices).

LIN_GRAPHS are the graphs of the debug_linearize test: (name, args, fixed). "tiny" is 3 vertices and 2 edges with the middle
vertex fixed, so both others hang on the fixed one alone.

LIN_GAPS[name] = (chi2, b, H_diag, H_off): the difference between sgraph_ref.linearize in fp64 and the same formulas in
numpy.longdouble (tools/sgraph_gap.py), chi2 relative, each array as max |difference| / max |entry|. The device is allowed
ten times each.
GAPS[name][k - 1] = (vertex, lambda, chi2_final): after k iterations, the largest absolute difference of any vertex entry and
the relative differences of lambda and chi2_final between the case's two runs of the restatement, measured on the CPU: the
pcg run and its OTHER run. OTHER is sgraph_ref.optimize(solver="direct"), and the device is allowed ten times each against
the direct solve. A case whose pcg_max_iters cuts the solver short ("pcgcap") has no direct solve to be near: its OTHER is
the same capped pcg run on the same graph with the edge list reversed (another summation order of the same sums), and the
device is allowed ten times each against the capped pcg run. MIN_RHO[name] is the smallest |rho| of any trial, and the margin
beside it is taken between the same two runs. EXEMPT cases have no margin on rho (it is 0, and NaN, by construction) and no
gap: they are compared exactly.
FIX_SCALE_GAP is the largest pose difference between sgraph_ref.optimize(fix_scale) and graph_ref.optimize on the SE(3) graph
"se3" (every scale 1) under the pcg solver, from the same tool; tests/test_sgraph_host.py allows ten times it.
All copied from the output of tools/sgraph_gap.py; the new seeds came from its --search."""
import collections
import functools
import re

import numpy as np

from aria_slam_amd import graph_ref as G
from aria_slam_amd import sgraph_ref as S
from graph_cases import CLAMP_RHO, update_factor      # noqa: F401  (the same LM control: tests/graph_cases.py beside this file)

Case = collections.namedtuple("Case", "name args fixed iterations fix_scale pattern handle note kind pcg_max_iters",
                              defaults=("random", 1000))

RHO_MIN = 1e-2             # every decision's |rho| is at least this ...
RHO_MARGIN = 1000.0        # ... and this many times the difference of that trial's rho between the case's two runs

CASES = [
    Case("random40", (31, 40, 12, 1.0), 0, 3, False, "AAA", None, "one random graph of 40 vertices"),
    Case("rejected", (31, 40, 12, 2.0), 0, 3, False, "rrrAAA", None, "three rejected trials before the first accept"),
    Case("fixed7", (34, 30, 8, 3.0), 7, 3, False, "rrrrAAA", None, "vertex 7 fixed"),
    Case("fixscale", (31, 40, 12, 2.0), 0, 3, True, "rrrAAA", None, "fix_scale on a graph whose scales are all 1"),
    Case("v513", (42, 513, 60, 3.0), 0, 2, False, "rrrrAA", (513, 1024), "513 vertices: a lane's second vertex"),
    Case("e513", (47, 200, 314, 3.0), 0, 2, False, "rrrAA", (256, 513), "513 edges: a lane's second edge"),
    # rejections after an accept: the W buffers have swapped (curW), the backup is of an accepted state, ni restarts at 2
    Case("separate", (107, 30, 8, 2.0), 0, 6, False, "AAArrArrrrAA", None,
         "rejections after 3 accepts (curW 1) and after 4 (curW 0), ni reaches 16, trials 11 and 12 (rho 0.974, 0.953) clamped"),
    # (seed 130 at noise 3, not 125 at 0.5 (AAAArAA): there the chi2 gap after 3 iterations, 4.1e-10, lies a hundred times below
    # those after 2 and 4, 4.4e-08 and 3.0e-08 -- the two solves' chi2 crossed there, which says nothing about the solvers, and
    # the device's solve, a third one that stops ten PCG iterations later, came to 1.8e-08. The restatement does the same on
    # the CPU: its pcg run in reversed summation order lies at 4.2e-09 there, and at half the tolerance at 1.9e-08
    # (tests/test_sgraph_host.py holds both, and every case of this table to the reversed run). tools/sgraph_gap.py --search
    # marks such graphs, MAX_SPREAD there says why)
    Case("clamp", (130, 30, 8, 3.0), 0, 6, False, "rrrAArrAAAA", None,
         "trial 11 (rho 1.042) takes the 1/3 clamp: lambda after 6 iterations is a third of lambda after 5; the five other "
         "accepts (rho 0.015 .. 0.896) do not; rejections after 2 accepts (curW 0)"),
    # rho == 0 exactly, and chi2 overflowing
    Case("exact", (12,), 0, 5, False, "r" * 10, None, "rho == 0 in all ten trials; lambda ends at lambda0 * 2^55", "exact"),
    Case("overflow", (31, 40, 12, 2.0, 1e306), 0, 3, False, "r" * 10, None, "chi2_initial = inf; rho is NaN in all ten trials",
         "overflow"),
    Case("fixscale_scaled", (31, 40, 12, 2.0), 13, 3, True, "rrrAAA", None, "fix_scale on scales in [0.5, 2], vertex 13 fixed",
         "scaled"),
    Case("topology", (2, 1.0), 0, 3, False, "AArA", (256, 512),
         "a hub of degree 210, a free vertex with no edge, an edge with info_scale 0, a pair joined three times", "topology"),
    Case("pcgcap", (31, 40, 12, 1.0), 0, 3, False, "AAA", None, "random40 with pcg_max_iters = 3: 9 solver iterations", "random", 3),
]
BY_NAME = {c.name: c for c in CASES}
EXEMPT = ("exact", "overflow")     # no margin on rho: it is 0, and NaN, by construction

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
    # separate direct AAArrArrrrAA pcg AAArrArrrrAA
    #   accepted rho 0.196 0.462 0.582 0.491 0.974 0.953
    "separate": [(7.05e-06, 1.79e-07, 1.20e-07), (9.85e-06, 1.97e-07, 1.06e-06), (1.31e-05, 1.61e-07, 5.22e-07),
                 (2.16e-05, 1.63e-07, 2.21e-06), (2.27e-05, 1.63e-07, 9.79e-07), (2.70e-05, 1.63e-07, 4.07e-07)],
    # clamp direct rrrAArrAAAA pcg rrrAArrAAAA
    #   accepted rho 0.015 0.550 0.896 0.481 0.860 1.042
    "clamp": [(8.10e-08, 8.06e-09, 2.47e-09), (1.80e-07, 7.37e-09, 1.68e-08), (2.12e-07, 5.41e-08, 1.41e-08),
              (2.14e-07, 5.41e-08, 2.05e-08), (2.05e-07, 1.32e-07, 3.68e-08), (2.02e-07, 1.32e-07, 3.26e-08)],
    # exact direct rrrrrrrrrr pcg rrrrrrrrrr, rho ['0.0']: exact comparison, no gap
    # overflow direct rrrrrrrrrr pcg rrrrrrrrrr, rho ['nan']: exact comparison, no gap
    # fixscale_scaled direct rrrAAA pcg rrrAAA
    #   accepted rho 0.345 0.423 0.210
    "fixscale_scaled": [(2.12e-07, 1.15e-08, 2.78e-08), (5.72e-07, 2.51e-09, 6.72e-08), (1.43e-06, 3.81e-07, 1.69e-07)],
    # topology direct AArA pcg AArA
    #   accepted rho 0.786 0.790 0.155
    "topology": [(4.71e-07, 2.14e-09, 2.10e-09), (4.67e-07, 4.55e-09, 1.55e-09), (4.36e-07, 4.39e-08, 5.19e-09)],
    # pcgcap reversed AAA pcg AAA
    #   accepted rho 0.829 0.870 0.823
    #   9 solver iterations in 3 trials; uncapped, the same graph takes 188 191 250 per trial
    "pcgcap": [(4.44e-15, 7.76e-16, 1.08e-15), (5.33e-15, 1.04e-14, 1.69e-15), (5.33e-15, 1.57e-14, 2.05e-15)],
}
MIN_RHO = {    # case: smallest |rho| of any trial    (smallest |rho| / |rho_other - rho_pcg|)
    "random40": 0.411,    # 1.03e+06
    "rejected": 0.055,    # 2.57e+06
    "fixed7": 0.078,    # 7.07e+05
    "fixscale": 0.102,    # 7.2e+05
    "v513": 0.026,    # 7.8e+06
    "e513": 0.241,    # 4.24e+06
    "separate": 0.070,    # 8.62e+03
    "clamp": 0.015,    # 2.17e+06
    "fixscale_scaled": 0.210,    # 9.36e+05
    "topology": 0.144,    # 2.68e+06
    "pcgcap": 0.823,    # 4.9e+14
}
FIX_SCALE_GAP = 1.10e-10    # largest pose entry difference, sgraph_ref fix_scale against graph_ref


TOPO_VERTICES, TOPO_HUB_DEGREE = 240, 210     # the "topology" graph: vertex 238 is the hub, vertex 239 has no edge


def _measured(rng, V, a, b, noise, scale_noise=0.05):
    """random_sgraph's measurement of the edge a -> b: the true relative similarity times a small random one."""
    Zs = S.mul(S.mul(S.inv(V[a]), V[b]), S.vertex_from_pose(G.random_pose(rng, noise, noise), 1.0 + rng.uniform(-scale_noise, scale_noise)))
    return (a, b, float(rng.uniform(0.5, 10.0)), S.pose_of(Zs)[:3], float(Zs[12]))


def topology_graph(seed, noise):
    """TOPO_VERTICES vertices with scales in [0.5, 2]: a chain over 0..237; the hub 238 joined to vertices 0..209, every third
    of those edges pointing at the hub and the others away from it, so its adjacency list holds both directions; vertex 239
    free and without an edge; the pair (3, 17) joined twice as 3 -> 17 and once as 17 -> 3, three measurements of their own;
    and the edge 5 -> 40 with info_scale 0.0."""
    rng = np.random.default_rng(seed)
    n, hub = TOPO_VERTICES, TOPO_VERTICES - 2
    V = np.array([S.vertex_from_pose(G.random_pose(rng, 2.0), rng.uniform(0.5, 2.0)) for _ in range(n)]).reshape(-1, 13)
    pairs = [(k, k + 1) for k in range(hub - 1)]
    pairs += [((k, hub) if k % 3 == 0 else (hub, k)) for k in range(TOPO_HUB_DEGREE)]
    pairs += [(3, 17), (3, 17), (17, 3), (5, 40)]
    edges = [_measured(rng, V, a, b, noise) for a, b in pairs]
    edges[-1] = edges[-1][:2] + (0.0,) + edges[-1][3:]
    return V, edges


@functools.lru_cache(maxsize=None)
def graph(name):
    """(vertices (V, 13), edges) of a case."""
    c = BY_NAME[name]
    if c.kind == "exact":
        n = c.args[0]
        V = np.array([S.make_vertex(np.eye(3), [0.5 * i, 0.25 * i, 0.0], 2.0 ** (i % 3 - 1)) for i in range(n)])
        rel = lambda a, b: S.mul(S.inv(V[a]), V[b])      # noqa: E731
        edges = [(i, i + 1, 1.0, S.pose_of(rel(i, i + 1))[:3], float(rel(i, i + 1)[12])) for i in range(n - 1)]
        edges.append((0, n - 1, 10.0, S.pose_of(rel(0, n - 1))[:3], float(rel(0, n - 1)[12])))
        return V, edges
    if c.kind == "overflow":
        V, edges = S.random_sgraph(*c.args[:4])
        return V, [e[:2] + (c.args[4],) + e[3:] for e in edges]
    if c.kind == "topology":
        return topology_graph(*c.args)
    if c.kind == "scaled":
        return S.random_sgraph(*c.args)
    assert c.kind == "random"
    if c.fix_scale:                                   # the metric map: every vertex and edge scale exactly 1
        return S.random_sgraph(*c.args, scale_range=(1.0, 1.0), scale_noise=0.0)
    return S.random_sgraph(*c.args)


@functools.lru_cache(maxsize=None)
def lin_graph(name):
    args, fixed = {n: (a, f) for n, a, f in LIN_GRAPHS}[name]
    V, E = S.random_sgraph(*args)
    return V, E, fixed


def other(name):
    """The second run a case's gap and margin are measured against (the header, GAPS)."""
    return "reversed" if BY_NAME[name].pcg_max_iters < 1000 else "direct"


@functools.lru_cache(maxsize=None)
def reference(name, k, solver):
    """sgraph_ref.optimize of a case after k iterations: (vertices, result dict with its trace). solver "reversed" is the pcg
    run on the same graph with the edge list reversed."""
    c = BY_NAME[name]
    V, E = graph(name)
    if solver == "reversed":
        E, solver = list(E)[::-1], "pcg"
    if c.kind != "overflow":
        return S.optimize(V, E, c.fixed, k, solver, pcg_max_iters=c.pcg_max_iters, fix_scale=c.fix_scale)
    with np.errstate(all="ignore"):               # this case alone computes with inf and NaN on purpose
        return S.optimize(V, E, c.fixed, k, solver, pcg_max_iters=c.pcg_max_iters, fix_scale=c.fix_scale)


@functools.lru_cache(maxsize=None)
def uncapped(name):
    """The result dict of a capped case's graph under the default pcg_max_iters: what the cap cuts short."""
    c = BY_NAME[name]
    V, E = graph(name)
    return S.optimize(V, E, c.fixed, c.iterations, "pcg", fix_scale=c.fix_scale)[1]


def pattern(res):
    return "".join("A" if t["accepted"] else "r" for t in res["trace"])


def accepts_before_rejections(pat):
    """The number of accepted trials before each run of rejected ones, and the longest run of rejected trials."""
    before = [pat[:m.start()].count("A") for m in re.finditer(r"r+", pat)]
    return before, max([len(m.group()) for m in re.finditer(r"r+", pat)], default=0)


def rel(a, b):
    """|a - b| / |b|; 0 where both are equal (0 == 0, inf == inf)."""
    return 0.0 if a == b else abs(a - b) / abs(b)


def gap(name, k):
    """(vertex, lambda, chi2_final) between the pcg run of the restatement and the case's other run after k iterations."""
    (Vd, rd), (Vp, rp) = reference(name, k, other(name)), reference(name, k, "pcg")
    return float(np.abs(Vp - Vd).max()), rel(rp["lambda_"], rd["lambda_"]), rel(rp["chi2_final"], rd["chi2_final"])


def rho_margin(name):
    """(smallest |rho| of any trial, smallest |rho| / |difference of that trial's rho between the case's two runs|)."""
    c = BY_NAME[name]
    d, p = (np.array([t["rho"] for t in reference(name, c.iterations, s)[1]["trace"]]) for s in (other(name), "pcg"))
    lo = np.minimum(np.abs(d), np.abs(p))
    return float(lo.min()), float((lo / np.maximum(np.abs(d - p), 1e-300)).min())


def se3_graph():
    """(poses, edges) of graph_ref and the same graph as Sim(3) vertices and edges with every scale 1."""
    poses, edges = G.random_graph(*SE3_GRAPH)
    return poses, edges, S.vertices_from_poses(poses), [e + (1.0,) for e in edges]
