"""SE(3) pose-graph optimisation on the MI355X (aria_graph_*, kernel in aria_slam_amd/csrc/graph_optimize.hip): the
linearisation and the LM run against the NumPy restatement (aria_slam_amd/graph_ref.py), loop closing, a consistent graph,
determinism over batch position and batch split, the edges of the input space, the adapters in Python and C++, and
euroc_frontend --optimize.

Tolerance of the LM comparison. The device runs block-Jacobi PCG capped at 1000 iterations and 1e-8; the yardstick is the
restatement with the direct solve. Measured on the CPU on this file's own graphs (GRAPHS below, 1 and 10 iterations), the
largest absolute difference of any pose entry between graph_ref(solver="direct") and graph_ref(solver="pcg") is
    circle1 1.8e-6   circle2 1.46e-5   circle3 1.7e-6   random7 1.3e-7   chain8 2.4e-7   floating9 1.3e-7
so GAP = 1.46e-5 and the device is allowed TOL = 10 * GAP = 1.46e-4 (metres or quaternion-sized rotation entries) against
the direct solve: one decade for a different summation order through ~1e3 CG steps. iterations_done, trials and stop_reason
are compared with graph_ref(solver="pcg"), the algorithm the device runs; pcg_iterations is printed, not asserted (a
different summation order moves a stop by a few iterations).

Graphs of more than 512 vertices take the kernel's strided solver instead of the one-vertex-per-lane one; circle4 (700
vertices, 3 loops) covers it. There the capped PCG lags the direct solve more: the CPU-measured gap is 1.01e-6 after 1
iteration and 1.24e-3 after 5 (every solve ends at the cap), so the device is allowed 1.01e-5 and 1.24e-2. dense22 (200
vertices, 599 edges) is one vertex per lane but too many edges for the on-chip form of that solver; its CPU-measured gap
after 1 iteration is 3.7e-8, so the device is allowed 3.7e-7.

The graphs above never make LM reject a trial. The rejected-trial path (the restore of the poses, lambda *= ni, ni *= 2, the
ni = 2 reset, the ten-trial stop) runs on the cases of tests/graph_cases.py, under the same convention: ten times the
CPU-measured direct-vs-pcg gap of that case after that many iterations (GAPS there, from tools/graph_gap.py) for the poses,
for lambda and for chi2_final, the discrete fields equal to the pcg restatement's. tests/test_graph_host.py proves on the CPU
that no decision of those cases is near enough to rho = 0 for the device's summation order to flip it."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import graph_cases as GC   # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "aria_slam_amd")
GAP = 1.46e-5
TOL = 10 * GAP
ARIA_E_INVALID, ARIA_E_TOO_LARGE = -1, -4


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def opt(aria):
    o = aria.HipPoseGraphOptimizer(max_vertices=512, max_edges=1024, max_graphs=4)
    yield o
    o.close()


def _graph(name):
    from aria_slam_amd import graph_ref as G
    if name.startswith("circle"):
        seed = int(name[6:])
        _truth, init, odo, loops = G.circle_scene(seed, n_loops=6 if seed == 2 else 1)
        return init, odo + loops
    if name == "random7":
        return G.random_graph(7, 60, 10)
    if name == "chain8":
        return G.random_graph(8, 25, 0)
    assert name == "floating9"          # vertices 30.. form a component that does not hang on the fixed vertex
    p, e = G.random_graph(9, 40, 6)
    return p, [x for x in e if (x[0] < 30) == (x[1] < 30)]


GRAPHS = ["circle1", "circle2", "circle3", "random7", "chain8", "floating9"]


def _fields(r):
    return tuple(r[k] for k in ("iterations_done", "trials", "stop_reason", "valid"))


# ---- linearisation ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,nv,extra", [(11, 40, 12), (12, 200, 30), (13, 3, 0)])
def test_linearisation_equals_the_restatement(opt, seed, nv, extra):
    from aria_slam_amd import graph_ref as G
    poses, edges = G.random_graph(seed, nv, extra, noise=0.3)
    edges = edges + [edges[0]]                                    # a duplicate edge is just another edge
    chi2, b, D, W = opt.debug_linearize(poses, edges, 0)
    c2, b2, D2, W2 = G.linearize(poses, edges)
    figs = dict(chi2=abs(chi2 - c2) / c2, b=np.abs(b - b2).max() / np.abs(b2).max(), D=np.abs(D - D2).max() / np.abs(D2).max(),
                W=np.abs(W - W2).max() / np.abs(W2).max())
    print("linearisation seed %d:" % seed, figs)
    assert all(v <= 1e-9 for v in figs.values()), figs


# ---- LM against the restatement -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GRAPHS)
def test_lm_equals_the_restatement(opt, name):
    from aria_slam_amd import graph_ref as G
    poses, edges = _graph(name)
    for its in (1, 10):
        P, r = opt.optimize_graph(poses, edges, 0, its)
        Pd, _rd = G.optimize(poses, edges, 0, its, "direct")
        Pp, rp = G.optimize(poses, edges, 0, its, "pcg")
        gap_direct, gap_pcg = np.abs(P - Pd).max(), np.abs(P - Pp).max()
        print("%s %d iterations: device vs direct %.3g, device vs pcg restatement %.3g, restatement pcg vs direct %.3g; "
              "chi2 %.6g -> %.6g, %d PCG iterations" % (name, its, gap_direct, gap_pcg, np.abs(Pp - Pd).max(), r["chi2_initial"],
                                                        r["chi2_final"], r["pcg_iterations"]))
        assert np.isfinite(P).all()
        assert gap_direct <= TOL, (name, its, gap_direct)
        assert _fields(r) == _fields(rp), (r, rp)
        # these graphs never reject a trial (trials == iterations_done); the ones that do are tests/graph_cases.py's, below
        assert r["iterations_done"] == its and r["stop_reason"] == G.STOP_ITERATIONS
        assert abs(r["chi2_initial"] - rp["chi2_initial"]) <= 1e-9 * rp["chi2_initial"]
        assert r["chi2_final"] <= r["chi2_initial"]
        assert P[0].tobytes() == np.asarray(poses)[0].tobytes()       # the fixed vertex is bitwise unchanged


def test_lm_equals_the_restatement_beyond_one_vertex_per_lane(aria):
    from aria_slam_amd import graph_ref as G
    _truth, init, odo, loops = G.circle_scene(4, n=700, laps=1.1, n_loops=3)
    edges = odo + loops
    big = aria.HipPoseGraphOptimizer(max_vertices=1024, max_edges=1024)
    for its, gap in ((1, 1.01e-6), (5, 1.24e-3)):
        P, r = big.optimize_graph(init, edges, 0, its)
        Pd, _rd = G.optimize(init, edges, 0, its, "direct")
        Pp, rp = G.optimize(init, edges, 0, its, "pcg")
        print("circle4 %d iterations: device vs direct %.3g, device vs pcg restatement %.3g, restatement pcg vs direct %.3g; "
              "chi2 %.6g -> %.6g, %d PCG iterations (restatement %d)" % (its, np.abs(P - Pd).max(), np.abs(P - Pp).max(),
                                                                         np.abs(Pp - Pd).max(), r["chi2_initial"], r["chi2_final"],
                                                                         r["pcg_iterations"], rp["pcg_iterations"]))
        assert np.abs(P - Pd).max() <= 10 * gap
        assert _fields(r) == _fields(rp) and r["iterations_done"] == its
        assert r["chi2_final"] < r["chi2_initial"] and P[0].tobytes() == init[0].tobytes()
    # the same graph in a batch beside small ones, and alone: bitwise identical
    small = G.random_graph(8, 25, 0)
    Pb, Rb, st = big.optimize_batch([(small[0], small[1], 0), (init, edges, 0), (small[0], small[1], 0)], 5)
    assert st == 0 and Pb[1].tobytes() == P.tobytes() and Rb[1]["record"] == r["record"]
    assert Pb[0].tobytes() == Pb[2].tobytes()
    big.close()


def test_lm_equals_the_restatement_with_more_edges_than_the_lds_holds(aria):
    from aria_slam_amd import graph_ref as G
    poses, edges = G.random_graph(22, 200, 400)
    assert len(edges) == 599
    o = aria.HipPoseGraphOptimizer(max_vertices=256, max_edges=640)
    P, r = o.optimize_graph(poses, edges, 0, 1)
    Pd, _rd = G.optimize(poses, edges, 0, 1, "direct")
    Pp, rp = G.optimize(poses, edges, 0, 1, "pcg")
    print("dense22 1 iteration: device vs direct %.3g, device vs pcg restatement %.3g; chi2 %.6g -> %.6g, %d PCG iterations "
          "(restatement %d)" % (np.abs(P - Pd).max(), np.abs(P - Pp).max(), r["chi2_initial"], r["chi2_final"],
                                r["pcg_iterations"], rp["pcg_iterations"]))
    assert np.abs(P - Pd).max() <= 10 * 3.7e-8 and _fields(r) == _fields(rp)
    assert r["chi2_final"] < r["chi2_initial"] and P[0].tobytes() == poses[0].tobytes()
    P5, r5 = o.optimize_graph(poses, edges, 0, 5)
    _P5, rp5 = G.optimize(poses, edges, 0, 5, "pcg")
    assert np.isfinite(P5).all() and _fields(r5) == _fields(rp5) and r5["chi2_final"] <= r["chi2_final"]
    o.close()


# ---- the rejected-trial path (tests/graph_cases.py) ------------------------------------------------------------------------------
def _handle_for(aria, opt, c):
    if c.handle is None:
        return opt
    return aria.HipPoseGraphOptimizer(max_vertices=c.handle[0], max_edges=c.handle[1])


@pytest.mark.parametrize("name", [c.name for c in GC.CASES if c.name not in GC.EXEMPT])
def test_rejected_trials_equal_the_restatement(aria, opt, name):
    """LM's state restarts at every call, so the runs of 1, 2, ..., K iterations pin the number of rejections before every
    accept, and lambda and chi2 after it."""
    from aria_slam_amd import graph_ref as G
    c = GC.BY_NAME[name]
    poses, edges = GC.graph(name)
    o = _handle_for(aria, opt, c)
    try:
        share = [0.0, 0.0, 0.0]
        for k in range(1, c.iterations + 1):
            P, r = o.optimize_graph(poses, edges, c.fixed, k)
            (Pd, rd), (Pp, rp) = GC.reference(name, k, "direct"), GC.reference(name, k, "pcg")
            got = (np.abs(P - Pd).max(), GC.rel(r["lambda_"], rd["lambda_"]), GC.rel(r["chi2_final"], rd["chi2_final"]))
            allowed = [10 * g for g in GC.GAPS[name][k - 1]]
            share = [max(s, g / a) for s, g, a in zip(share, got, allowed)]
            print("%s %d iterations, %s: device vs direct pose %.3g lambda %.3g chi2 %.3g (allowed %.3g %.3g %.3g), device vs pcg "
                  "restatement pose %.3g lambda %.3g; trials %d, %d PCG iterations (restatement %d)"
                  % (name, k, GC.pattern(rp), *got, *allowed, np.abs(P - Pp).max(), GC.rel(r["lambda_"], rp["lambda_"]), r["trials"],
                     r["pcg_iterations"], rp["pcg_iterations"]))
            assert np.isfinite(P).all()
            assert _fields(r) == _fields(rp), (k, r, rp)
            assert r["iterations_done"] == k and r["stop_reason"] == G.STOP_ITERATIONS
            assert got[0] <= allowed[0], (k, got, allowed)
            assert got[1] <= allowed[1], (k, got, allowed)
            assert got[2] <= allowed[2], (k, got, allowed)
            assert abs(r["chi2_initial"] - rp["chi2_initial"]) <= 1e-9 * rp["chi2_initial"]
            assert P[c.fixed].tobytes() == poses[c.fixed].tobytes()       # the fixed vertex is bitwise unchanged
        assert r["trials"] == len(c.pattern)
        print("%s: largest share of the allowance: pose %.3g lambda %.3g chi2_final %.3g" % (name, *share))
    finally:
        if o is not opt:
            o.close()


def test_an_exact_minimum_rejects_ten_zero_steps(opt):
    """chi2 = 0 and b = 0: every trial is a zero step with rho == 0, which `rho > 0` rejects. lambda0 is 1e-5 times a sum of
    products of multiples of 1/4 (exact in fp64 in any order) and every later factor is a power of two, so lambda is
    compared exactly."""
    from aria_slam_amd import graph_ref as G
    c = GC.BY_NAME["exact"]
    poses, edges = GC.graph(c.name)
    for k in (1, c.iterations):
        P, r = opt.optimize_graph(poses, edges, c.fixed, k)
        _Pp, rp = GC.reference(c.name, k, "pcg")
        print("exact minimum, %d iterations:" % k, {f: r[f] for f in r if f != "record"})
        assert P.tobytes() == poses.tobytes()
        assert _fields(r) == _fields(rp) and (r["trials"], r["iterations_done"]) == (10, 0)
        assert r["stop_reason"] == G.STOP_TRIALS and r["valid"] == 1
        assert r["chi2_initial"] == 0.0 and r["chi2_final"] == 0.0
        assert r["lambda_"] == rp["lambda_"] == 3963167672086.0366


def test_an_overflowing_chi2_rejects_every_trial_and_returns_the_poses(opt):
    """Every info_scale is 1e306 (finite, valid): chi2 is inf at the input and inf or NaN after any step, so every trial
    fails the finiteness guard whatever the solver does with the non-finite system. Only what the restatement fixes is
    asserted: the discrete fields and the poses, bitwise. The loops it runs are the ten trials and the capped PCG."""
    from aria_slam_amd import graph_ref as G
    c = GC.BY_NAME["overflow"]
    poses, edges = GC.graph(c.name)
    g = _graph("chain8")
    P0, r0 = opt.optimize_graph(g[0], g[1], 0, 3)
    for k in (1, c.iterations):
        P, r = opt.optimize_graph(poses, edges, c.fixed, k)
        _Pp, rp = GC.reference(c.name, k, "pcg")
        print("overflow, %d iterations:" % k, {f: r[f] for f in r if f != "record"})
        assert P.tobytes() == poses.tobytes()
        assert _fields(r) == _fields(rp) == (0, 10, G.STOP_TRIALS, 1)
    # nothing non-finite stays behind in the handle's scratch: a gentle graph is bitwise what it was before
    P1, r1 = opt.optimize_graph(g[0], g[1], 0, 3)
    assert P1.tobytes() == P0.tobytes() and r1["record"] == r0["record"] and r1["iterations_done"] == 3


# ---- it closes loops ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,n_loops", [(1, 1), (2, 6), (3, 1)])
def test_it_closes_loops(opt, seed, n_loops):
    """300 vertices on 1.1 laps of a 5 m circle with 0.2 m vertical ripple, odometry noise 0.001 rad / 0.005 m per step and a
    yaw bias of 0.0008 rad per step, loop edges one lap apart at 10x information, 10 iterations."""
    from aria_slam_amd import graph_ref as G
    truth, init, odo, loops = G.circle_scene(seed, n=300, laps=1.1, radius=5.0, ripple=0.2, rot_noise=0.001, trans_noise=0.005,
                                             yaw_bias=0.0008, n_loops=n_loops)
    assert len(loops) == n_loops and all(e[2] == 10.0 for e in loops)
    P, r = opt.optimize_graph(init, odo + loops, 0, 10)
    a0, a1 = G.ate(init, truth), G.ate(P, truth)
    print("seed %d: chi2 %.4g -> %.4g, ATE %.3f -> %.3f m (ratio %.2f)" % (seed, r["chi2_initial"], r["chi2_final"], a0, a1, a1 / a0))
    assert r["valid"] == 1 and r["chi2_final"] < 1e-3 * r["chi2_initial"]
    assert a1 <= 0.7 * a0
    assert P[0].tobytes() == init[0].tobytes()


# ---- a consistent graph stays put ------------------------------------------------------------------------------------------------------
def test_a_consistent_graph_stays_put(opt):
    from aria_slam_amd import graph_ref as G
    _truth, _init, odo, _loops = G.circle_scene(5, n=200)
    chain = [G.random_pose(np.random.default_rng(5), 2.0)]
    for (_i, _j, _s, Z) in odo:
        chain.append(chain[-1] @ Z)
    chain = np.array(chain)
    P, r = opt.optimize_graph(chain, odo, 0, 10)
    print("consistent graph: moved %.3g, chi2 %.3g -> %.3g" % (np.abs(P - chain)[:, :3, 3].max(), r["chi2_initial"], r["chi2_final"]))
    assert np.abs(P - chain)[:, :3, 3].max() < 1e-9 and np.abs(P - chain).max() < 1e-9
    assert r["chi2_final"] <= r["chi2_initial"] and r["valid"] == 1
    assert P[0].tobytes() == chain[0].tobytes()


# ---- determinism ------------------------------------------------------------------------------------------------------------------
def test_batch_position_split_and_rerun_are_bitwise_identical(aria, opt, torch_cuda):
    from aria_slam_amd import graph_ref as G
    A = _graph("circle1")
    others = [_graph("random7"), _graph("chain8"), G.random_graph(21, 150, 20), _graph("floating9")]
    g = lambda pe, fixed=0: (pe[0], pe[1], fixed)
    batch = [g(A), g(A), g(others[0]), g(others[1], 3), g(others[2]), g(others[3]), g(A)]        # A at 0, 1 and B-1
    P, R, st = opt.optimize_batch(batch, 6)
    assert st == 0 and all(r["valid"] == 1 for r in R)
    for k in (1, 6):
        assert P[k].tobytes() == P[0].tobytes() and R[k]["record"] == R[0]["record"]
    # alone, through the single-graph entry point
    Ps, Rs = opt.optimize_graph(A[0], A[1], 0, 6)
    assert Ps.tobytes() == P[0].tobytes() and Rs["record"] == R[0]["record"]
    # the batch split in two calls, and on a handle with one slot (every graph its own launch)
    P1, R1, _ = opt.optimize_batch(batch[:3], 6)
    P2, R2, _ = opt.optimize_batch(batch[3:], 6)
    one = aria.HipPoseGraphOptimizer(max_vertices=512, max_edges=1024, max_graphs=1)
    P3, R3, _ = one.optimize_batch(batch, 6)
    one.close()
    # the same call again
    P4, R4, _ = opt.optimize_batch(batch, 6)
    for k in range(len(batch)):
        for Pk, Rk in (((P1 + P2)[k], (R1 + R2)[k]), (P3[k], R3[k]), (P4[k], R4[k])):
            assert Pk.tobytes() == P[k].tobytes() and Rk["record"] == R[k]["record"], k
        assert P[k][batch[k][2]].tobytes() == np.asarray(batch[k][0])[batch[k][2]].tobytes()     # fixed vertices


def test_a_rejecting_graph_is_bitwise_identical_wherever_it_runs(aria, opt, torch_cuda):
    """A graph whose LM rejects (separate104: rrrrAArAArA) alone, first, in the middle and last in a batch beside graphs that
    never reject, in a split batch and on a handle with one slot: its poses and record are the same bits everywhere, and its
    neighbours are bitwise what they are without it."""
    c = GC.BY_NAME["separate104"]
    R = GC.graph(c.name) + (c.fixed,)
    its = c.iterations
    others = [_graph("random7") + (0,), _graph("chain8") + (3,), _graph("floating9") + (0,)]
    P0, r0 = opt.optimize_graph(R[0], R[1], R[2], its)
    _Pp, rp = GC.reference(c.name, its, "pcg")
    assert _fields(r0) == _fields(rp) and r0["trials"] == len(c.pattern) > r0["iterations_done"] == its
    Pn, Rn, st = opt.optimize_batch(others, its)                     # the neighbours without it
    assert st == 0 and all(r["trials"] == r["iterations_done"] == its for r in Rn)
    one = aria.HipPoseGraphOptimizer(max_vertices=512, max_edges=1024, max_graphs=1)
    for pos in range(len(others) + 1):
        batch = others[:pos] + [R] + others[pos:]
        where = [k for k in range(len(batch)) if k != pos]
        runs = [opt.optimize_batch(batch, its)[:2]]
        Pa, Ra, _ = opt.optimize_batch(batch[:2], its)               # split in two calls
        Pb, Rb, _ = opt.optimize_batch(batch[2:], its)
        runs.append((Pa + Pb, Ra + Rb))
        runs.append(one.optimize_batch(batch, its)[:2])              # every graph its own launch
        for P, Rs in runs:
            assert P[pos].tobytes() == P0.tobytes() and Rs[pos]["record"] == r0["record"], pos
            for k, n in zip(where, range(len(others))):
                assert P[k].tobytes() == Pn[n].tobytes() and Rs[k]["record"] == Rn[n]["record"], (pos, k)
    P1, R1, _ = one.optimize_batch([R], its)                         # alone in a batch call, alone on the one-slot handle
    P2, R2, _ = opt.optimize_batch([R], its)
    one.close()
    assert P1[0].tobytes() == P2[0].tobytes() == P0.tobytes() and R1[0]["record"] == R2[0]["record"] == r0["record"]
    # more graphs than slots: the handle's own split into launches, the rejecting graph in each of them
    batch = [R, others[0], others[1], others[2], others[1], R, others[0]]
    P, Rs, st = opt.optimize_batch(batch, its)
    assert st == 0
    for k in (0, 5):
        assert P[k].tobytes() == P0.tobytes() and Rs[k]["record"] == r0["record"]
    for k, n in ((1, 0), (2, 1), (3, 2), (4, 1), (6, 0)):
        assert P[k].tobytes() == Pn[n].tobytes() and Rs[k]["record"] == Rn[n]["record"]


# ---- the edges of the input space ------------------------------------------------------------------------------------------------------
def test_edges_of_the_input_space(aria, opt, torch_cuda):
    from aria_slam_amd import graph_ref as G
    poses, edges = _graph("random7")
    # no edges: every trial is a zero step; nothing moves (the restatement's rule)
    P, r = opt.optimize_graph(poses, [], 0, 5)
    _Pr, rr = G.optimize(poses, [], 0, 5)
    assert P.tobytes() == poses.tobytes() and _fields(r) == _fields(rr) and r["stop_reason"] == G.STOP_TRIALS
    assert r["chi2_initial"] == r["chi2_final"] == 0.0
    # one vertex; no vertex
    P, r = opt.optimize_graph(poses[:1], [], 0, 5)
    assert P.tobytes() == poses[:1].tobytes() and r["valid"] == 1
    P, r = opt.optimize_graph(poses[:0], [], 0, 5)
    assert len(P) == 0 and r["valid"] == 1
    # iterations = 0: poses bitwise unchanged, chi2_final == chi2_initial
    P, r = opt.optimize_graph(poses, edges, 0, 0)
    assert P.tobytes() == poses.tobytes() and r["chi2_final"] == r["chi2_initial"] > 0 and r["trials"] == 0
    # duplicate edges: as the restatement
    dup = edges + edges[:5]
    P, r = opt.optimize_graph(poses, dup, 0, 3)
    Pd, _ = G.optimize(poses, dup, 0, 3, "direct")
    Pp, rp = G.optimize(poses, dup, 0, 3, "pcg")
    assert np.abs(P - Pd).max() <= TOL and _fields(r) == _fields(rp)
    # another fixed vertex
    P, r = opt.optimize_graph(poses, edges, 17, 3)
    Pd, _ = G.optimize(poses, edges, 17, 3, "direct")
    assert np.abs(P - Pd).max() <= TOL and P[17].tobytes() == poses[17].tobytes()

    # an edge index out of range: that graph only, ARIA_E_INVALID from check, the neighbours bitwise as without it
    other = _graph("chain8")
    bad_edges = list(edges)
    bad_edges[4] = (bad_edges[4][0], len(poses), bad_edges[4][2], bad_edges[4][3])
    clean = [(other[0], other[1], 0), (poses, edges, 0), (other[0], other[1], 2)]
    Pc, Rc, st = opt.optimize_batch(clean, 4)
    assert st == 0
    for bad in ((poses, bad_edges, 0), (poses, edges, len(poses)), (poses, [(3, 3, 1.0, np.eye(4))], 0),
                (poses, [(0, 1, float("nan"), np.eye(4))], 0), (poses, [(-1, 1, 1.0, np.eye(4))], 0)):
        Pb, Rb, st = opt.optimize_batch([clean[0], bad, clean[2]], 4, raise_on_error=False)
        assert st == ARIA_E_INVALID
        assert Rb[1]["valid"] == 0 and Rb[1]["stop_reason"] == G.STOP_INVALID and Pb[1].tobytes() == poses.tobytes()
        for k in (0, 2):
            assert Pb[k].tobytes() == Pc[k].tobytes() and Rb[k]["record"] == Rc[k]["record"]
        assert opt.status() == 0                                   # reported once
        with pytest.raises(aria.AriaError) as ei:                  # the host entry point refuses it before any launch
            opt.optimize_graph(*bad, 4)
        assert ei.value.status == ARIA_E_INVALID

    # a graph larger than the handle
    small = aria.HipPoseGraphOptimizer(max_vertices=32, max_edges=64, max_graphs=2)
    Pb, Rb, st = small.optimize_batch([clean[0], (poses, edges, 0), clean[2]], 4, raise_on_error=False)
    assert st == ARIA_E_TOO_LARGE and Rb[1]["valid"] == 0 and Pb[1].tobytes() == poses.tobytes()
    for k in (0, 2):
        assert Pb[k].tobytes() == Pc[k].tobytes() and Rb[k]["record"] == Rc[k]["record"]
    with pytest.raises(aria.AriaError) as ei:
        small.optimize_graph(poses, edges, 0, 4)
    assert ei.value.status == ARIA_E_TOO_LARGE
    big_e = [other[1][k % len(other[1])] for k in range(65)]       # 25 vertices, 65 edges: too many edges
    with pytest.raises(aria.AriaError) as ei:
        small.optimize_graph(other[0], big_e, 0, 4)
    assert ei.value.status == ARIA_E_TOO_LARGE
    small.close()


# ---- the adapters ------------------------------------------------------------------------------------------------------------------
def _fmt(M):
    return " ".join("%.17g" % v for v in np.asarray(M, np.float64).reshape(16))


def test_python_and_cpp_adapters_against_each_other_and_the_restatement(aria, tmp_path):
    """The reference-shaped methods with sparse ids (0, 1, 2, 5, 6): edges to the missing ids 3 and 4 are dropped; the first
    id added (2) is the fixed vertex; a re-added id overwrites; loop edges weigh 10x."""
    from aria_slam_amd import graph_ref as G
    rng = np.random.default_rng(31)
    ids = [2, 0, 1, 5, 6]
    truth = {k: G.random_pose(rng, 2.0) for k in range(7)}
    calls = []
    for k in ids:
        calls.append(("P", k, truth[k] @ G.random_pose(rng, 0.1, 0.05)))
    calls.append(("P", 5, truth[5] @ G.random_pose(rng, 0.1, 0.05)))                  # overwrite
    for a in range(6):                                                             # 2-3, 3-4, 4-5 name missing ids
        calls.append(("O", a, a + 1, 1.0 + 0.5 * a, G.inv(truth[a]) @ truth[a + 1] @ G.random_pose(rng, 0.01, 0.01)))
    calls.append(("L", 6, 0, 1.0, G.inv(truth[6]) @ truth[0]))
    calls.append(("L", 5, 2, 2.0, G.inv(truth[5]) @ truth[2]))
    calls.append(("L", 4, 0, 1.0, np.eye(4)))                                       # dropped
    calls.append(("O", 2, 5, 1.0, G.inv(truth[2]) @ truth[5]))

    py, ref = aria.HipPoseGraphOptimizer(max_vertices=64, max_edges=64), G.PoseGraphOptimizer()
    lines = []
    for c in calls:
        for o in (py, ref):
            if c[0] == "P":
                o.set_initial_pose(c[1], c[2])
            elif c[0] == "O":
                o.add_odometry_edge(c[1], c[2], c[4], c[3])
            else:
                o.add_loop_edge(c[1], c[2], c[4], c[3])
        op = "LC" if c[0] == "L" and c[1] == 5 else c[0]            # one loop edge goes in the way the driver adds them
        lines.append("P %d %s" % (c[1], _fmt(c[2])) if op == "P" else "%s %d %d %.17g %s" % (op, c[1], c[2], c[3], _fmt(c[4])))
    assert len(py.poses) == 5 and len(py.edges) == 6 and [e[:3] for e in py.edges] == [e[:3] for e in ref.edges]
    assert sorted(e[2] for e in py.edges)[-2:] == [10.0, 20.0]
    py.optimize(10)
    ref.optimize(10)
    lines += ["OPT 10"] + ["GET %d" % k for k in range(8)] + ["ALL", "CLEAR", "GET 2", "ALL"]
    script = tmp_path / "script.txt"
    script.write_text("\n".join(lines) + "\n")

    subprocess.check_call(["make", "-C", os.path.join(PKG, "host"), "-s"])
    exe = os.path.join(ROOT, "build", "graph_selftest")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "host", "include"),
                           os.path.join(ROOT, "tests", "cpp", "graph_selftest.cpp"), "-o", exe, "-L" + PKG, "-laria_hip_adapters",
                           "-laria_orb_hip", "-lz", "-Wl,-rpath," + PKG])
    out = subprocess.run([exe, str(script)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "DONE" in out.stdout, out.stdout + out.stderr
    rows = [l.split() for l in out.stdout.splitlines()]
    got = [(int(r[1]), np.array(r[2:], np.float64).reshape(4, 4)) for r in rows if r[0] == "pose"]
    assert [k for k, _ in got] == list(range(8)) + [2] and np.array_equal(got[8][1], np.eye(4))    # after clear(): the identity
    cpp = dict(got[:8])
    allp = [np.array(r[2:], np.float64).reshape(4, 4) for r in rows if r[0] == "allpose"]
    res = [r for r in rows if r[0] == "result"][0]
    # C++ == Python bitwise (the same library on the same arrays); both within TOL of the restatement
    for k in range(8):
        want = py.get_optimized_pose(k)
        assert cpp[k].tobytes() == want.tobytes(), k
        assert np.abs(want - ref.get_optimized_pose(k)).max() <= TOL
        if k in (3, 4, 7):
            assert np.array_equal(want, np.eye(4))                 # unknown ids: the identity
    assert py.get_optimized_pose(2).tobytes() == [c for c in calls if c[0] == "P" and c[1] == 2][0][2].tobytes()   # fixed = first added
    r = py.last_result
    assert [float(res[1]), float(res[2])] == [r["chi2_initial"], r["chi2_final"]]
    assert [int(x) for x in res[3:]] == [r["iterations_done"], r["trials"], r["pcg_iterations"], r["valid"], r["stop_reason"]]
    assert _fields(r) == _fields(ref.last_result) and r["chi2_final"] < r["chi2_initial"]
    assert [r for r in rows if r[0] == "all"] == [["all", "5"], ["all", "0"]]
    assert [p.tobytes() for p in allp] == [p.tobytes() for p in py.get_all_poses()]            # ascending id order
    assert [p.tobytes() for p in py.get_all_poses()] == [py.get_optimized_pose(k).tobytes() for k in (0, 1, 2, 5, 6)]
    assert [r for r in rows if r[0] == "graph"] == [["graph", "0", "0"]]
    py.clear()
    assert py.get_all_poses() == [] and np.array_equal(py.get_optimized_pose(2), np.eye(4))
    py.optimize(3)                                                 # an empty graph: nothing happens
    py.close()


def test_euroc_frontend_optimize(aria, tmp_path):
    """--optimize FILE: refused without --pose / --loop-verify reference; one line per frame; with no accepted loop the file
    equals the --pose file to 1e-9; the --pose file and the CSV are byte-identical with and without the flag."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_frontend_io import _make_dataset
    subprocess.check_call(["make", "-C", os.path.join(PKG, "host"), "-s"])
    seq, _ = _make_dataset(aria, str(tmp_path), 8, w=640, h=480)
    exe = os.path.join(PKG, "euroc_frontend")
    p1, p2, c1, c2, o2 = (str(tmp_path / n) for n in ("p1.txt", "p2.txt", "c1.csv", "c2.csv", "opt.txt"))
    base = [exe, str(tmp_path), "1000", "--loop", "--loop-verify", "reference"]
    for bad in ([exe, str(tmp_path), "1000", "--optimize", o2], [exe, str(tmp_path), "1000", "--pose", p1, "--optimize", o2],
                [exe, str(tmp_path), "1000", "--pose", p1, "--loop", "--optimize", o2]):
        r = subprocess.run(bad, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "--optimize needs" in r.stderr
    plain = subprocess.run(base + ["--pose", p1, "--csv", c1], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0, plain.stdout + plain.stderr
    run = subprocess.run(base + ["--pose", p2, "--csv", c2, "--optimize", o2], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert open(p1, "rb").read() == open(p2, "rb").read() and open(c1, "rb").read() == open(c2, "rb").read()
    line = [l for l in run.stdout.splitlines() if l.startswith("pose graph ")]
    assert len(line) == 1 and not [l for l in plain.stdout.splitlines() if l.startswith("pose graph ")]
    print(line[0])
    n_vertices = int(line[0].split()[2])
    updates = int([l for l in run.stdout.splitlines() if l.startswith("pose updates ")][0].split()[2])
    assert n_vertices == updates > 0                              # one vertex per accepted pose (euroc_eval.cpp:211-215)
    assert "loops 0" in run.stdout                                 # 16 frames: no loop candidate, so no loop edge
    a = np.array([l.split() for l in open(p2).read().splitlines()], np.float64)
    b = np.array([l.split() for l in open(o2).read().splitlines()], np.float64)
    assert a.shape == b.shape == (len(seq), 8)
    assert np.array_equal(a[:, 0], b[:, 0]) and np.abs(a - b).max() <= 1e-9
