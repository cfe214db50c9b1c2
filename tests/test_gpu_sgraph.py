"""Sim(3) pose-graph optimisation and map correction on the MI355X (aria_sgraph_*, kernels in aria_slam_amd/csrc/sim3_graph.hip)
against the NumPy restatement (aria_slam_amd/sgraph_ref.py): the linearisation, the LM run at every iteration count of the cases
of tests/sgraph_cases.py, bitwise identity over batch position and split, the edges of the input space, the closed walk whose
scale drift the stage exists for, the map correction bit for bit, and the copy kernels.

Tolerances are the tables of tests/sgraph_cases.py, measured on the CPU by tools/sgraph_gap.py: ten times the restatement's
fp64-to-long-double gap for debug_linearize, ten times its direct-vs-pcg gap for the LM run (the device differs from the pcg
run by rounding only). tests/test_sgraph_host.py proves on the CPU that no decision of a case is near enough to rho = 0 for
the device's summation order to flip it."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sgraph_cases as SC                                              # noqa: E402
from test_sgraph_host import WALK_REF, _points                         # noqa: E402

pytestmark = pytest.mark.gpu

ARIA_E_INVALID, ARIA_E_TOO_LARGE = -1, -4


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


# ---- linearisation ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n, _a, _f in SC.LIN_GRAPHS])
def test_linearisation_equals_the_restatement(opt, name):
    from aria_slam_amd import sgraph_ref as S
    V, E, fixed = SC.lin_graph(name)
    chi2, b, D, W = opt.debug_linearize(V, E, fixed)
    c2, b2, D2, W2 = S.linearize(V, S.norm_edges(E))
    figs = (abs(chi2 - c2) / c2, np.abs(b - b2).max() / np.abs(b2).max(), np.abs(D - D2).max() / np.abs(D2).max(),
            np.abs(W - W2).max() / np.abs(W2).max())
    print("linearisation %s: chi2 %.3g b %.3g H_diag %.3g H_off %.3g; allowed %s" % ((name,) + figs + (
        tuple(10 * g for g in SC.LIN_GAPS[name]),)))
    for got, gap in zip(figs, SC.LIN_GAPS[name]):
        assert got <= 10 * gap, (name, figs, SC.LIN_GAPS[name])
    assert np.array_equal(D, np.transpose(D, (0, 2, 1)))              # the diagonal blocks are symmetric bit for bit


# ---- LM against the restatement -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in SC.CASES if c.name not in SC.EXEMPT])
def test_lm_equals_the_restatement_at_every_iteration_count(aria, opt, name):
    """LM's state restarts at every call, so the runs of 1, 2, ..., K iterations pin the number of rejections before every
    accept, and lambda and chi2 after it. The run the device is held to is the direct solve; for a case whose pcg_max_iters
    cuts the solver short it is the capped pcg run (tests/sgraph_cases.py, GAPS)."""
    c = SC.BY_NAME[name]
    V, E = SC.graph(name)
    capped = SC.other(name) == "reversed"
    o = opt
    if c.handle or c.fix_scale or c.pcg_max_iters != 1000:
        mv, me = c.handle or (512, 1024)
        o = aria.HipSim3GraphOptimizer(max_vertices=mv, max_edges=me, fix_scale=c.fix_scale, pcg_max_iters=c.pcg_max_iters)
    try:
        share = [0.0, 0.0, 0.0]
        for k in range(1, c.iterations + 1):
            P, r = o.optimize_graph(V, E, c.fixed, k)
            _Pp, rp = SC.reference(name, k, "pcg")
            Pd, rd = (_Pp, rp) if capped else SC.reference(name, k, "direct")
            gv, gl, gc = SC.GAPS[name][k - 1]
            figs = (float(np.abs(P - Pd).max()), SC.rel(r["lambda_"], rd["lambda_"]), SC.rel(r["chi2_final"], rd["chi2_final"]))
            share = [max(s, f / (10 * g)) for s, f, g in zip(share, figs, (gv, gl, gc))]
            print("%s k=%d %s: vertex %.3g lambda %.3g chi2 %.3g; allowed %.3g %.3g %.3g; device vs pcg restatement %.3g; %d PCG "
                  "iterations (restatement %d)" % ((name, k, SC.pattern(rp)) + figs + (10 * gv, 10 * gl, 10 * gc,
                                                                                    float(np.abs(P - _Pp).max()),
                                                                                    r["pcg_iterations"], rp["pcg_iterations"])))
            assert np.isfinite(P).all()
            assert figs[0] <= 10 * gv and figs[1] <= 10 * gl and figs[2] <= 10 * gc, (name, k, figs)
            assert SC.MIN_RHO[name] >= SC.RHO_MIN                     # the margin the table records: the discrete fields hold
            assert _fields(r) == _fields(rp), (r, rp)
            assert r["iterations_done"] == k and r["stop_reason"] == 0
            assert abs(r["chi2_initial"] - rp["chi2_initial"]) <= 1e-12 * rp["chi2_initial"]
            assert P[c.fixed].tobytes() == V[c.fixed].tobytes()       # the fixed vertex is never written
            if c.fix_scale:
                assert P[:, 12].tobytes() == V[:, 12].tobytes()       # every s bit for bit
            if capped:
                assert r["pcg_iterations"] == c.pcg_max_iters * r["trials"] == rp["pcg_iterations"]
        assert r["trials"] == len(c.pattern)
        print("%s: largest share of the allowance: vertex %.3g lambda %.3g chi2_final %.3g" % ((name,) + tuple(share)))
    finally:
        if o is not opt:
            o.close()


# ---- bitwise identity -----------------------------------------------------------------------------------------------------------------
def test_bitwise_identity_over_batch_position_split_and_rerun(aria, opt):
    V, E = SC.graph("rejected")
    other = [SC.graph("random40"), SC.graph("fixed7")]
    alone, r = opt.optimize_graph(V, E, 0, 3)
    again, r2 = opt.optimize_graph(V, E, 0, 3)
    assert alone.tobytes() == again.tobytes() and r["record"] == r2["record"]
    fill = [(other[0][0], other[0][1], 0), (other[1][0], other[1][1], 7), (other[0][0], other[0][1], 0)]
    first = [(V, E, 0)] + fill + [(other[1][0], other[1][1], 7)]
    last = [(other[1][0], other[1][1], 7)] + fill + [(V, E, 0)]
    one = aria.HipSim3GraphOptimizer(max_vertices=512, max_edges=1024, max_graphs=1)
    try:
        for o in (opt, one):                                          # max_graphs 4 and 1: a batch of 5 is split 4 + 1 and 1 x 5
            Pf, Rf, st = o.optimize_batch(first, 3)
            Pl, Rl, st2 = o.optimize_batch(last, 3)
            assert st == 0 and st2 == 0
            assert Pf[0].tobytes() == alone.tobytes() == Pl[4].tobytes()
            assert Rf[0]["record"] == r["record"] == Rl[4]["record"]
            assert Pf[4].tobytes() == Pl[0].tobytes() and Pf[1].tobytes() == Pf[3].tobytes()
    finally:
        one.close()


# ---- the input space --------------------------------------------------------------------------------------------------------------------
def test_edges_of_the_input_space(opt):
    from aria_slam_amd import sgraph_ref as S
    V, E = SC.graph("random40")
    # an empty graph, and one vertex with no edge
    P, r = opt.optimize_graph(np.zeros((0, 13)), [], 0, 3)
    assert len(P) == 0 and r["valid"] == 1 and r["trials"] == 0
    P, r = opt.optimize_graph(V[:1], [], 0, 3)
    _Pr, rr = S.optimize(V[:1], [], 0, 3)
    assert P.tobytes() == V[:1].tobytes() and _fields(r) == _fields(rr)
    # iterations = 0 writes nothing
    P, r = opt.optimize_graph(V, E, 0, 0)
    assert P.tobytes() == V.tobytes() and r["trials"] == 0 and r["chi2_final"] == r["chi2_initial"] > 0


def _bad_graphs():
    """what -> (vertices, edges, fixed): everything the kernel's validation refuses besides the counts and the sizes."""
    V, E = SC.graph("random40")
    E = list(E)
    nv = len(V)
    self_edge = E[:3] + [(5, 5, 1.0, np.eye(4), 1.0)] + E[3:]

    def edge4(**kw):                                                  # the table's edges with fields of edge 4 replaced
        e = dict(zip(("a", "b", "w", "Z", "s"), E[4]))
        e.update(kw)
        return E[:4] + [(e["a"], e["b"], e["w"], e["Z"], e["s"])] + E[5:]

    def vertex9(s):
        Vb = V.copy()
        Vb[9, 12] = s
        return Vb
    return {"self-edge": (V, self_edge, 0), "edge s = 0": (V, edge4(s=0.0), 0), "edge s = NaN": (V, edge4(s=float("nan")), 0),
            "edge s = +Inf": (V, edge4(s=float("inf")), 0), "info_scale < 0": (V, edge4(w=-1.0), 0),
            "info_scale NaN": (V, edge4(w=float("nan")), 0), "info_scale +Inf": (V, edge4(w=float("inf")), 0),
            "edge index -1": (V, edge4(a=-1), 0), "edge index nv": (V, edge4(b=nv), 0),
            "vertex s = 0": (vertex9(0.0), E, 0), "vertex s = NaN": (vertex9(np.nan), E, 0), "vertex s = +Inf": (vertex9(np.inf), E, 0),
            "fixed == -1": (V, E, -1), "fixed == nv": (V, E, nv), "0 vertices, 1 edge": (V[:0], E[:1], 0)}


BAD = ["self-edge", "edge s = 0", "edge s = NaN", "edge s = +Inf", "info_scale < 0", "info_scale NaN", "info_scale +Inf",
       "edge index -1", "edge index nv", "vertex s = 0", "vertex s = NaN", "vertex s = +Inf", "fixed == -1", "fixed == nv",
       "0 vertices, 1 edge"]


@pytest.mark.parametrize("what", ["negative count"] + BAD + ["too large"])
def test_a_bad_graph_in_a_batch_leaves_its_neighbours_alone(torch_cuda, opt, what):
    from aria_slam_amd import _lib
    from aria_slam_amd.simgraph import pack_sim3_edges, pack_vertices
    torch = torch_cuda
    assert sorted(BAD) == sorted(_bad_graphs())
    good = [SC.graph("random40"), SC.graph("rejected")]
    want, want_r, st = opt.optimize_batch([(good[0][0], good[0][1], 0), (good[1][0], good[1][1], 0)], 2)
    assert st == 0
    fixed_b = 0
    if what == "too large":
        Vb, Eb = SC.graph("v513")                                     # 513 vertices against a handle of 512
    elif what == "negative count":
        Vb, Eb = good[0]
    else:
        Vb, Eb, fixed_b = _bad_graphs()[what]
    rows = [pack_vertices(good[0][0]), pack_vertices(Vb), pack_vertices(good[1][0])]
    recs = [pack_sim3_edges(good[0][1]), pack_sim3_edges(Eb), pack_sim3_edges(good[1][1])]
    voff = np.concatenate([[0], np.cumsum([len(x) for x in rows])]).astype(np.int32)
    eoff = np.concatenate([[0], np.cumsum([len(x) for x in recs])]).astype(np.int32)
    if what == "negative count":
        # the buffers hold graph 2 first, then graph 0; the offsets run n2, n2 + n0, 0, n2: graph 1 owns [n2 + n0, 0), a negative
        # count of vertices and of edges, and graphs 0 and 2 own what is theirs
        rows, recs = [rows[2], rows[0]], [recs[2], recs[0]]
        voff = np.array([len(rows[0]), len(rows[0]) + len(rows[1]), 0, len(rows[0])], np.int32)
        eoff = np.array([len(recs[0]), len(recs[0]) + len(recs[1]), 0, len(recs[0])], np.int32)
        rows.insert(1, rows[0][:0])                                   # what "graph 1" wrote must be nothing: an empty slice
    dev = torch.device("cuda", 0)
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev)      # noqa: E731
    allrows, allrecs = np.concatenate(rows), np.concatenate(recs)
    dp, dv, de, do, df = d(allrows), d(voff), d(allrecs), d(eoff), d(np.array([0, fixed_b, 0], np.int32))
    dres = torch.zeros(3 * _lib.SGRAPH_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    opt.optimize_batch_device(dp, dv, de, do, df, 3, 2, dres)
    status = opt.status()
    assert status == (ARIA_E_TOO_LARGE if what == "too large" else ARIA_E_INVALID)
    assert opt.status() == 0                                          # reported once
    out = np.frombuffer(dp.cpu().numpy().tobytes(), np.float64).reshape(-1, 13)
    res = np.frombuffer(dres.cpu().numpy().tobytes(), _lib.SGRAPH_RESULT_DTYPE)
    assert out[voff[0]:voff[1]].tobytes() == want[0].tobytes() and res[0].tobytes() == want_r[0]["record"]
    assert out[voff[2]:voff[3]].tobytes() == want[1].tobytes() and res[2].tobytes() == want_r[1]["record"]
    assert res[1]["valid"] == 0 and res[1]["stop_reason"] == 2 and res[1]["trials"] == 0
    assert out[voff[1]:voff[2]].tobytes() == rows[1].tobytes()        # nothing of the bad graph is written


def test_the_host_form_refuses_what_the_kernel_refuses(opt):
    from aria_slam_amd import AriaError
    for what, (V, E, fixed) in _bad_graphs().items():
        with pytest.raises(AriaError):
            opt.optimize_graph(V, E, fixed, 2)
        with pytest.raises(AriaError):
            opt.debug_linearize(V, E, fixed)
    V, E = SC.graph("v513")
    with pytest.raises(AriaError):
        opt.optimize_graph(V, E, 0, 2)
    assert opt.status() == 0


def test_an_information_scale_of_minus_zero_is_valid(opt):
    """info_scale == -0.0 passes `>= 0` in the kernel, on the host and in the restatement. Its edge contributes -0.0 where
    +0.0 would contribute +0.0; added to the sums of a vertex that has other edges, either leaves every bit as it was, so
    the run is that of info_scale == +0.0 bit for bit, in the restatement and on the device."""
    from aria_slam_amd import sgraph_ref as S
    V, E = SC.graph("random40")
    Em, Ez = list(E), list(E)
    Em[4], Ez[4] = E[4][:2] + (-0.0,) + E[4][3:], E[4][:2] + (0.0,) + E[4][3:]
    Pm, rm = opt.optimize_graph(V, Em, 0, 3)
    Pz, rz = opt.optimize_graph(V, Ez, 0, 3)
    Sm, sm = S.optimize(V, Em, 0, 3, "pcg")
    Sz, _sz = S.optimize(V, Ez, 0, 3, "pcg")
    assert sm["valid"] == 1 and Sm.tobytes() == Sz.tobytes()
    assert rm["valid"] == 1 and _fields(rm) == _fields(sm) and rm["iterations_done"] == 3
    assert Pm.tobytes() == Pz.tobytes() and rm["record"] == rz["record"]
    assert not np.array_equal(Pm, V) and opt.status() == 0


# ---- the walk ---------------------------------------------------------------------------------------------------------------------------
def test_the_walk_on_the_device(aria, opt):
    """tools/sgraph_walk.py's walk with the exact loop edge: the device's ATE is at most twice WALK_REF (the margin
    tests/test_cpp_sim3.py gives the same walk) and strictly below the device SE(3) graph's on the same edge; the map correction
    of the two triangulated pairs moves the arena bit for bit as sgraph_ref.correct_points does."""
    import sgraph_walk as SW
    import sim3_walk as W
    from aria_slam_amd import sgraph_ref as S
    from aria_slam_amd._lib import MATCH_DTYPE
    w = SW.walk()
    K, L = W.K_FRAMES, W.K_FRAMES - 1
    Z, s = w["exact"]
    se3 = aria.HipPoseGraphOptimizer(max_vertices=64, max_edges=64)
    for g in (opt, se3):
        g.clear()
        for i in range(K):
            g.set_initial_pose(i, w["c2w"][i])
        for i, j, _w, Zo in w["odo"]:
            g.add_odometry_edge(i, j, Zo)
    opt.add_loop_edge(0, L, Z, s)
    se3.add_loop_edge(0, L, Z)
    old = opt.vertices()
    opt.optimize(SW.ITERATIONS)
    se3.optimize(SW.ITERATIONS)
    new = opt.vertices()
    ate7, ate6 = SW.ate(SW.centres(np.array(opt.poses)), w["truth"]), SW.ate(SW.centres(np.array(se3.poses)), w["truth"])
    law = W.DRIFT ** (-np.arange(K) / (K - 1.0))
    print("device walk: ATE sim3 %s, se3 %s, WALK_REF %s, scales off the law by %.3e" % (ate7, ate6, WALK_REF,
                                                                                         np.abs(np.array(opt.scales) - law).max()))
    assert ate7[0] <= 2 * WALK_REF[0] and ate7[1] <= 2 * WALK_REF[1]
    assert ate7[0] < ate6[0] and ate7[1] < ate6[1]
    se3.close()
    # the two pairs triangulated on the device, then corrected where they lie
    m = aria.HipMapper(capacity=1024)
    ident = np.zeros(W.N_POINTS, MATCH_DTYPE)
    ident["query_idx"] = ident["train_idx"] = np.arange(W.N_POINTS)
    f, dr = w["frames"], w["drifted"]
    m.triangulate(f[0], f[1], ident, dr[0], dr[1], pair_id=0)
    m.triangulate(f[L - 1], f[L], ident, dr[L - 1], dr[L], pair_id=1)
    before = m.read()
    assert len(before) > 100 and set(before["pair"]) == {0, 1}
    stats, status = opt.correct_map(m, w["pair_vertex"], 0, old, new)
    after = m.read()
    want, want_stats = S.correct_points(before, w["pair_vertex"], 0, old, new)
    assert status == 0 and stats == want_stats == (len(before), 0, 0)
    assert after.tobytes() == want.tobytes()
    assert not np.array_equal(after["X"], before["X"])
    m.close()
    opt.clear()


# ---- the correction, bitwise ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_correction_is_the_restatements_bit_for_bit(opt, n):
    from aria_slam_amd import graph_ref as G
    from aria_slam_amd import sgraph_ref as S
    rng = np.random.default_rng(n)
    old = np.array([S.vertex_from_pose(G.random_pose(rng, 2.0), rng.uniform(0.5, 2)) for _ in range(4)])
    new = np.array([S.vertex_from_pose(G.random_pose(rng, 2.0), rng.uniform(0.5, 2)) for _ in range(4)])
    pts = _points(n, [3, 4, 5, 6, 7, 9], seed=n)                       # pair 3 below pair_base, 9 beyond the table
    table = [0, -1, 3, 2]                                              # pairs 4..7: hits, and a -1
    got, stats, status = opt.correct_points(pts, table, 4, old, new)
    want, want_stats = S.correct_points(pts, table, 4, old, new)
    assert status == 0 and stats == want_stats and sum(stats) == n and stats[2] == 0
    assert got.tobytes() == want.tobytes()
    # one vertex with s <= 0: its points are refused and counted, the error is deferred, the others move as before
    bad = new.copy()
    bad[3, 12] = -0.5
    got_b, stats_b, status_b = opt.correct_points(pts, table, 4, old, bad, raise_on_error=False)
    want_b, want_stats_b = S.correct_points(pts, table, 4, old, bad)
    assert stats_b == want_stats_b and got_b.tobytes() == want_b.tobytes()
    assert status_b == (ARIA_E_INVALID if want_stats_b[2] else 0) and opt.status() == 0
    hit3 = pts["pair"] == 6
    assert got_b[hit3].tobytes() == pts[hit3].tobytes() and got_b[~hit3].tobytes() == got[~hit3].tobytes()
    # every byte outside X is unchanged
    raw_in = pts.view(np.uint8).reshape(n, -1)
    for rec in (got, got_b):
        raw = rec.view(np.uint8).reshape(n, -1)
        assert np.array_equal(raw[:, :8], raw_in[:, :8]) and np.array_equal(raw[:, 32:], raw_in[:, 32:])


# ---- copies ---------------------------------------------------------------------------------------------------------------------------
def test_copy_kernels_round_trip_bit_for_bit(torch_cuda, opt):
    from aria_slam_amd import _lib
    torch = torch_cuda
    rng = np.random.default_rng(7)
    n = 300
    rows = rng.normal(size=(n, 12))
    rows[5, 3] = -0.0
    rows[6, 7] = np.nan                                               # integer copies: any bit pattern survives
    dev = torch.device("cuda", 0)
    d_rows = torch.from_numpy(rows.copy()).to(dev)
    d_v = torch.zeros(n * 13, dtype=torch.float64, device=dev)
    d_back = torch.zeros(n * 12, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    opt.vertices_from_pose_device(d_rows, d_v, n)
    opt.poses_from_vertices_device(d_v, d_back, n)
    opt.check()
    v = np.frombuffer(d_v.cpu().numpy().tobytes(), _lib.SGRAPH_VERTEX_DTYPE)
    r3 = rows.reshape(n, 3, 4)
    assert v["R"].tobytes() == np.ascontiguousarray(r3[:, :, :3]).tobytes() and v["t"].tobytes() == np.ascontiguousarray(r3[:, :, 3]).tobytes()
    assert (v["s"] == 1.0).all()
    assert d_back.cpu().numpy().tobytes() == rows.tobytes()
