"""The paths of the Sim(3) pose-graph stage (kernels in aria_slam_amd/csrc/sim3_graph.hip) that tests/test_gpu_sgraph.py's
table runs do not assert by themselves, on the MI355X against the NumPy restatement (aria_slam_amd/sgraph_ref.py): ten zero
steps at an exact minimum and STOP_TRIALS, a chi2 that overflows, one launch over graphs of very different sizes, and the map
correction at a size that takes a second trip of its stride loop, with every form of refusal and with the empty tables.

The inputs are those of tests/sgraph_cases.py; tests/test_sgraph_host.py proves on the CPU that they are what their notes say."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sgraph_cases as SC                                              # noqa: E402
from test_sgraph_host import _points                                   # noqa: E402

pytestmark = pytest.mark.gpu

ARIA_E_INVALID = -1
STOP_TRIALS = 1
CORRECT_LANES = 4096 * 256          # the correction's launch is capped at this many lanes


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def opt(aria):
    o = aria.HipSim3GraphOptimizer(max_vertices=512, max_edges=1024, max_graphs=4)
    yield o
    o.close()


def _fields(r):
    return tuple(r[k] for k in ("iterations_done", "trials", "stop_reason", "valid"))


# ---- STOP_TRIALS ----------------------------------------------------------------------------------------------------------------------
def test_an_exact_minimum_rejects_ten_zero_steps(opt):
    """chi2 = 0 and b = 0: the solver returns dx = 0 after 0 iterations (|b| = 0), every trial is a zero step with rho == 0,
    which `rho > 0` rejects, and the tenth ends the call. Every entry of the graph is a multiple of a power of two small
    enough for the sums of H's diagonal to be exact in any order, and every factor of lambda after lambda0 is a power of two,
    so lambda is compared exactly."""
    from aria_slam_amd import sgraph_ref as S
    c = SC.BY_NAME["exact"]
    V, E = SC.graph("exact")
    _c2, _b, D, _W = S.linearize(V, S.norm_edges(E))
    lam0 = 1e-5 * max(D[v, k, k] for v in range(len(V)) if v != c.fixed for k in range(7))
    for k in range(1, c.iterations + 1):
        P, r = opt.optimize_graph(V, E, c.fixed, k)
        _Pp, rp = SC.reference("exact", k, "pcg")
        print("exact minimum, %d iterations:" % k, {f: r[f] for f in r if f != "record"})
        assert P.tobytes() == V.tobytes()
        assert _fields(r) == _fields(rp) == (0, 10, STOP_TRIALS, 1)
        assert r["chi2_initial"] == 0.0 and r["chi2_final"] == 0.0
        assert r["lambda_"] == rp["lambda_"] == lam0 * 2.0 ** 55
        assert r["pcg_iterations"] == 0


def test_an_overflowing_chi2_rejects_every_trial_and_returns_the_vertices(opt):
    """Every info_scale is 1e306 (finite, valid): chi2 is inf at the input and inf or NaN after any step, so every trial fails
    the finiteness guard whatever the solver makes of the non-finite system (tests/graph_cases.py's header). Only what the
    restatement fixes is asserted: the discrete fields, chi2_initial and the vertices, bitwise."""
    c = SC.BY_NAME["overflow"]
    V, E = SC.graph("overflow")
    g = SC.graph("random40")
    P0, r0 = opt.optimize_graph(g[0], g[1], 0, 2)
    for k in range(1, c.iterations + 1):
        P, r = opt.optimize_graph(V, E, c.fixed, k)
        _Pp, rp = SC.reference("overflow", k, "pcg")
        print("overflow, %d iterations:" % k, {f: r[f] for f in r if f != "record"})
        assert P.tobytes() == V.tobytes()
        assert _fields(r) == _fields(rp) == (0, 10, STOP_TRIALS, 1)
        assert r["chi2_initial"] == rp["chi2_initial"] == np.inf
    # nothing non-finite stays behind in the handle's scratch: a gentle graph is bitwise what it was before
    P1, r1 = opt.optimize_graph(g[0], g[1], 0, 2)
    assert P1.tobytes() == P0.tobytes() and r1["record"] == r0["record"] and r1["iterations_done"] == 2


# ---- one launch, four sizes -------------------------------------------------------------------------------------------------------------
def test_graphs_of_different_sizes_in_one_launch_equal_their_runs_alone(aria):
    """513 vertices (a lane's second vertex) beside 3 vertices, 40 vertices and the empty graph, on a handle of four slots sized
    for the largest: one launch, every workgroup with its own trip counts. Each result is the graph's alone, bit for bit."""
    big, tiny, mid = SC.graph("v513"), SC.lin_graph("tiny"), SC.graph("random40")
    graphs = [(big[0], big[1], 0), (tiny[0], tiny[1], tiny[2]), (mid[0], mid[1], 0), (np.zeros((0, 13)), [], 0)]
    assert [len(g[0]) for g in graphs] == [513, 3, 40, 0]
    o = aria.HipSim3GraphOptimizer(max_vertices=513, max_edges=1024, max_graphs=4)
    try:
        alone = [o.optimize_graph(V, E, fixed, 2) for V, E, fixed in graphs]
        P, R, status = o.optimize_batch(graphs, 2)
        assert status == 0
        for k, (Pa, ra) in enumerate(alone):
            assert P[k].tobytes() == Pa.tobytes() and R[k]["record"] == ra["record"], k
        assert [r["valid"] for r in R] == [1, 1, 1, 1] and [r["trials"] for r in R][3] == 0
        assert R[0]["iterations_done"] == R[1]["iterations_done"] == R[2]["iterations_done"] == 2
        assert not np.array_equal(P[0], big[0]) and not np.array_equal(P[1], tiny[0])
        Pr, Rr, status = o.optimize_batch(graphs[::-1], 2)            # the same four in the other slots
        assert status == 0 and all(Pr[3 - k].tobytes() == P[k].tobytes() and Rr[3 - k]["record"] == R[k]["record"] for k in range(4))
    finally:
        o.close()


# ---- the correction ---------------------------------------------------------------------------------------------------------------------
def _similarities(n, seed):
    from aria_slam_amd import graph_ref as G
    from aria_slam_amd import sgraph_ref as S
    rng = np.random.default_rng(seed)
    make = lambda: np.array([S.vertex_from_pose(G.random_pose(rng, 2.0), rng.uniform(0.5, 2)) for _ in range(n)])      # noqa: E731
    return make(), make()


def test_correction_takes_a_second_trip_of_the_stride_loop(opt):
    """More points than the launch has lanes: the first 257 lanes move a second point each."""
    from aria_slam_amd import sgraph_ref as S
    n = CORRECT_LANES + 257
    old, new = _similarities(4, 11)
    pts = _points(n, [3, 4, 5, 6, 7, 9, 4], seed=11)                   # pair 3 below pair_base, 9 beyond the table; period 7
    assert pts.dtype.itemsize == 72
    pts["pair"][CORRECT_LANES:] = [4] * 100 + [5] * 57 + [6] * 100     # the second trip: hits, -1s, hits
    table = [0, -1, 3, 2]                                              # pairs 4..7
    got, stats, status = opt.correct_points(pts, table, 4, old, new)
    want, want_stats = S.correct_points(pts, table, 4, old, new)
    print("correction of %d points: (moved, left alone, refused) %s" % (n, stats))
    assert status == 0 and stats == want_stats and sum(stats) == n and stats[2] == 0 and min(stats[:2]) > n // 8
    assert got.tobytes() == want.tobytes()
    tail = slice(CORRECT_LANES, n)
    moved = np.isin(pts["pair"][tail], [4, 6])
    assert moved.sum() == 200 and not (got["X"][tail][moved] == pts["X"][tail][moved]).all(1).any()
    assert got[tail][~moved].tobytes() == pts[tail][~moved].tobytes()


def test_correction_refuses_every_bad_entry_and_moves_the_others(opt):
    """Vertices 0..3 are good; 4..7 have a bad old scale (0, negative, NaN, +Inf) and a good new one, 8..11 the other way
    round. The table names them all, and n_vertices itself, an index far beyond, -1 and another negative index. Nine points of
    good vertices carry a NaN, a +Inf or a -Inf in one coordinate each."""
    from aria_slam_amd import sgraph_ref as S
    nv, n = 12, 360
    old, new = _similarities(nv, 12)
    clean_old, clean_new = old.copy(), new.copy()
    for k, bad in enumerate((0.0, -0.5, np.nan, np.inf)):
        old[4 + k, 12] = bad
        new[8 + k, 12] = bad
    table = list(range(nv)) + [nv, 1 << 30, -1, -7]                    # pairs 10..25
    pts = _points(n, list(range(8, 28)), seed=12)                      # pairs 8, 9 below pair_base; 26, 27 beyond the table
    clean = pts.copy()
    at = np.flatnonzero(np.isin(pts["pair"], [10, 11, 12, 13]))[:9]    # points of the good vertices
    for k, i in enumerate(at):
        pts["X"][i, k % 3] = (np.nan, np.inf, -np.inf)[k // 3]
    got, stats, status = opt.correct_points(pts, table, 10, old, new, raise_on_error=False)
    want, want_stats = S.correct_points(pts, table, 10, old, new)
    per_pair = n // 20
    assert want_stats == (4 * per_pair - 9, 6 * per_pair, 10 * per_pair + 9)
    assert stats == want_stats and got.tobytes() == want.tobytes()
    assert status == ARIA_E_INVALID and opt.status() == 0              # reported once
    refused = np.isin(pts["pair"], list(range(14, 24)))
    refused[at] = True
    left = np.isin(pts["pair"], [8, 9, 24, 25, 26, 27])
    assert got[refused | left].tobytes() == pts[refused | left].tobytes()       # NaN payloads and all: bit for bit
    # the others move as they do without the bad entries
    got_c, stats_c, status_c = opt.correct_points(clean, table[:nv], 10, clean_old, clean_new)
    assert status_c == 0 and stats_c == (12 * per_pair, 8 * per_pair, 0)
    moved = ~(refused | left)
    assert moved.sum() == stats[0] and got[moved].tobytes() == got_c[moved].tobytes()
    assert not (got["X"][moved] == pts["X"][moved]).all(1).any()


def test_correction_with_an_empty_table_no_vertices_and_no_stats(torch_cuda, opt):
    from aria_slam_amd import sgraph_ref as S
    from aria_slam_amd._lib import MAP_POINT_DTYPE
    torch = torch_cuda
    old, new = _similarities(4, 13)
    pts = _points(300, [0, 1, 2, 3], seed=13)
    # n_table == 0: every point is left alone
    got, stats, status = opt.correct_points(pts, [], 0, old, new)
    assert status == 0 and stats == S.correct_points(pts, [], 0, old, new)[1] == (0, 300, 0) and got.tobytes() == pts.tobytes()
    # n_vertices == 0 with a table of -1 only
    none = np.zeros((0, 13))
    got, stats, status = opt.correct_points(pts, [-1, -1, -1, -1], 0, none, none)
    assert status == 0 and stats == S.correct_points(pts, [-1, -1, -1, -1], 0, none, none)[1] == (0, 300, 0)
    assert got.tobytes() == pts.tobytes()
    # ... and with a table that names a vertex: refused, as the restatement has it
    got, stats, status = opt.correct_points(pts, [-1, 0, -1, -1], 0, none, none, raise_on_error=False)
    assert stats == S.correct_points(pts, [-1, 0, -1, -1], 0, none, none)[1] == (0, 225, 75)
    assert status == ARIA_E_INVALID and got.tobytes() == pts.tobytes() and opt.status() == 0
    # d_stats == NULL: the points still move
    _t, dev, (dt, do, dn), n_table, nv, _dstats = opt._upload_correction([0, 1, 2, 3], old, new)
    dp = torch.from_numpy(pts.view(np.uint8).reshape(-1).copy()).to(dev)
    torch.cuda.synchronize(dev)
    opt.correct_points_device(dp, len(pts), dt, n_table, 0, do, dn, nv, None)
    assert opt.status() == 0
    out = np.frombuffer(dp.cpu().numpy().tobytes(), MAP_POINT_DTYPE)
    want, want_stats = S.correct_points(pts, [0, 1, 2, 3], 0, old, new)
    assert want_stats == (300, 0, 0) and out.tobytes() == want.tobytes() and not np.array_equal(out["X"], pts["X"])
