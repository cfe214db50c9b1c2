"""SE(3) pose-graph optimisation (include/aria_orb_hip.h, "SE(3) pose-graph optimisation"): the parts that need no GPU --
exports and layouts, the NumPy restatement (aria_slam_amd/graph_ref.py: the SE(3) pieces, the Jacobians against central
differences, PCG against the direct solve, LM's monotone chi2, the reference class's bookkeeping), the case table of the
rejected-trial path (tests/graph_cases.py: pattern, margin and coverage, proved with the restatement alone), the kernel's
listing and the C++ adapter build."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import graph_cases as GC       # noqa: E402
import isa_kernel_stats as S   # noqa: E402

GRAPH_SYMBOLS = ["aria_graph_default_config", "aria_graph_create", "aria_graph_destroy", "aria_graph_stream", "aria_graph_check",
                 "aria_graph_optimize", "aria_graph_optimize_batch_device", "aria_graph_debug_linearize"]


def test_graph_symbols_exported_and_listed(aria):
    from aria_slam_amd import _lib
    L = aria.load_library()
    header = open(os.path.join(ROOT, "include", "aria_orb_hip.h")).read()
    for name in GRAPH_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), "%s not declared in the header" % name
        assert hasattr(L, name), "libaria_orb_hip.so does not export %s" % name
        assert name in _lib.EXPORTS, "%s missing from _lib.EXPORTS" % name
    assert aria.abi_version() == 4
    assert aria.HipPoseGraphOptimizer


def _c_sizeof(tmp_path):
    """sizeof of the three structs as a C compiler sees the header."""
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "aria_orb_hip.h"\nint main(void) { printf("%zu %zu %zu\\n", '
                   'sizeof(aria_graph_config), sizeof(aria_graph_edge), sizeof(aria_graph_result)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    return [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]


def test_graph_record_layouts_and_defaults(aria, tmp_path):
    from aria_slam_amd import _lib
    cfg_size, edge_size, res_size = _c_sizeof(tmp_path)
    assert C.sizeof(_lib.GraphConfig) == cfg_size == 40
    assert C.sizeof(_lib.GraphEdge) == _lib.GRAPH_EDGE_DTYPE.itemsize == edge_size == 112
    assert C.sizeof(_lib.GraphResult) == _lib.GRAPH_RESULT_DTYPE.itemsize == res_size == 48
    cfg = _lib.GraphConfig()
    aria.load_library().aria_graph_default_config(C.byref(cfg))
    assert cfg.struct_size == 40 and cfg.max_graphs == 1 and cfg.pcg_max_iters == 1000 and cfg.pcg_rel_tol == 1e-8
    assert cfg.max_vertices == 4096 and cfg.max_edges == 8192


# ---- graph_ref: SE(3) -------------------------------------------------------------------------------------------------------
def test_mqt_round_trip_and_update_rules():
    from aria_slam_amd import graph_ref as G
    rng = np.random.default_rng(0)
    for _ in range(50):
        d = np.concatenate([rng.normal(size=3) * 3, rng.normal(size=3) * 0.4])
        if d[3:] @ d[3:] >= 1:
            continue
        assert np.abs(G.to_mqt(G.from_mqt(d)) - d).max() < 1e-15
    # |q|^2 > 1: the quaternion (0, -q) normalised, a half turn about -q
    T = G.from_mqt([0, 0, 0, 2.0, 0, 0])
    assert np.allclose(T[:3, :3], np.diag([1.0, -1, -1]), atol=1e-15)
    # every branch of quat_from_rot gives back the rotation, w >= 0
    for axis, ang in (([1, 0, 0], 3.1), ([0, 1, 0], 3.1), ([0, 0, 1], 3.1), ([1, 2, 3], 0.3), ([1, 1, 0], np.pi)):
        R = G.rot_axis(axis, ang)
        q = G.quat_from_rot(R)
        assert q[3] >= 0 and abs(q @ q - 1) < 1e-15 and np.abs(G.rot_from_quat(q) - R).max() < 1e-14
    # the update re-orthonormalises: a slightly non-orthogonal rotation comes out orthogonal
    X = G.random_pose(rng)
    X[:3, :3] += 1e-6 * rng.normal(size=(3, 3))
    Y = G.oplus(X, np.zeros(6))
    assert np.abs(Y[:3, :3] @ Y[:3, :3].T - np.eye(3)).max() < 1e-15
    assert np.array_equal(Y[:3, 3], X[:3, 3])


def test_analytic_jacobians_against_central_differences():
    from aria_slam_amd import graph_ref as G
    rng = np.random.default_rng(1)
    worst = 0.0
    for k in range(40):
        Xi, Xj = G.random_pose(rng, 3.0), G.random_pose(rng, 3.0)
        # small and large residual rotations: Z near the true relative pose, and anywhere
        Z = G.inv(Xi) @ Xj @ G.random_pose(rng, 0.1, 0.1) if k % 2 else G.random_pose(rng, 3.0)
        e, Ji, Jj = G.edge_jacobians(Xi, Xj, Z)
        assert np.array_equal(e, G.edge_error(Xi, Xj, Z))
        if G.quat_from_rot((G.inv(Z) @ G.inv(Xi) @ Xj)[:3, :3])[3] < 1e-3:
            continue                      # at w = 0 the sign choice makes the error discontinuous
        ni, nj = G.numeric_jacobians(Xi, Xj, Z)
        worst = max(worst, np.abs(Ji - ni).max(), np.abs(Jj - nj).max())
    # central differences with h = 1e-6 on entries of size <= ~10: truncation h^2 |f'''| ~ 1e-11, rounding 1e-16 / h ~ 1e-9
    assert worst < 1e-7, worst


def test_linearize_is_the_sum_over_edges_and_chi2_matches():
    from aria_slam_amd import graph_ref as G
    poses, edges = G.random_graph(3, 12, 5)
    chi2, b, D, W = G.linearize(poses, edges)
    assert abs(chi2 - G.chi2_of(poses, edges)) < 1e-12 * max(chi2, 1)
    assert np.allclose(D, np.transpose(D, (0, 2, 1)), atol=1e-12)
    # directional derivative of chi2 along a random update = -2 b.d
    rng = np.random.default_rng(0)
    d = rng.normal(size=(12, 6)) * 1e-6
    moved = np.array([G.oplus(poses[v], d[v]) for v in range(12)])
    moved_back = np.array([G.oplus(poses[v], -d[v]) for v in range(12)])
    num = (G.chi2_of(moved, edges) - G.chi2_of(moved_back, edges)) / 2
    assert abs(num - (-2 * (b * d).sum())) < 1e-6 * abs(num) + 1e-12


# ---- graph_ref: solvers and LM --------------------------------------------------------------------------------------------------
def test_pcg_against_direct_on_one_system():
    from aria_slam_amd import graph_ref as G
    _truth, init, odo, loops = G.circle_scene(4, n=120, n_loops=2)
    edges = odo + loops
    chi2, b, D, W = G.linearize(init, edges)
    lam = 1e-5 * max(D[v, k, k] for v in range(1, 120) for k in range(6))
    xd, _ = G.direct(D, W, edges, b, lam, 0)
    xp, iters = G.pcg(D, W, edges, b, lam, 0, 5000, 1e-12)
    assert 0 < iters < 5000
    assert not xp[0].any() and not xd[0].any()                  # the fixed vertex does not move
    assert np.abs(xp - xd).max() <= 1e-7 * np.abs(xd).max()
    # the cap is honoured and reported
    _x, capped = G.pcg(D, W, edges, b, lam, 0, 7, 1e-12)
    assert capped == 7
    # b = 0: nothing to do
    x0, it0 = G.pcg(D, W, edges, np.zeros_like(b), lam, 0)
    assert it0 == 0 and not x0.any()


@pytest.mark.parametrize("solver", ["direct", "pcg"])
def test_lm_chi2_never_increases_and_closes_the_loop(solver):
    from aria_slam_amd import graph_ref as G
    truth, init, odo, loops = G.circle_scene(1, n=150, n_loops=2)
    P, r = G.optimize(init, odo + loops, 0, 8, solver)
    hist = [r["chi2_initial"]] + r["chi2_history"]
    assert all(b <= a for a, b in zip(hist, hist[1:])), hist
    assert r["iterations_done"] == len(r["chi2_history"]) == 8 and r["stop_reason"] == G.STOP_ITERATIONS
    assert r["chi2_final"] < 1e-3 * r["chi2_initial"]
    assert G.ate(P, truth) < G.ate(init, truth)
    assert P[0].tobytes() == init[0].tobytes()                  # the fixed vertex
    assert (r["pcg_iterations"] > 0) == (solver == "pcg")


def test_lm_edges_of_the_input_space():
    from aria_slam_amd import graph_ref as G
    poses, edges = G.random_graph(2, 10, 3)
    # iterations = 0: nothing moves
    P, r = G.optimize(poses, edges, 0, 0)
    assert P.tobytes() == poses.tobytes() and r["chi2_final"] == r["chi2_initial"] and r["trials"] == 0
    # no edges: every trial is a zero step, the iteration fails, the call ends
    P, r = G.optimize(poses, [], 0, 5)
    assert P.tobytes() == poses.tobytes() and r["stop_reason"] == G.STOP_TRIALS and r["trials"] == G.MAX_TRIALS
    assert r["iterations_done"] == 0 and r["chi2_final"] == 0
    # one vertex
    P, r = G.optimize(poses[:1], [], 0, 5)
    assert P.tobytes() == poses[:1].tobytes() and r["valid"] == 1
    # invalid: an index out of range, a self-edge, a bad fixed index
    for bad_edges, fixed in (([(0, 10, 1.0, np.eye(4))], 0), ([(3, 3, 1.0, np.eye(4))], 0), ([], 10)):
        P, r = G.optimize(poses, bad_edges, fixed, 5)
        assert r["valid"] == 0 and r["stop_reason"] == G.STOP_INVALID and P.tobytes() == poses.tobytes()
    # a component that does not hang on the fixed vertex: finite poses from both solvers
    cut = [e for e in edges if (e[0] < 6) == (e[1] < 6)]
    for solver in ("pcg", "direct"):
        P, r = G.optimize(poses, cut, 0, 5, solver)
        assert np.isfinite(P).all() and r["valid"] == 1 and r["chi2_final"] <= r["chi2_initial"]
    # a consistent graph stays put
    chain = [poses[0]]
    for (_i, _j, _s, Z) in edges[:9]:
        chain.append(chain[-1] @ Z)
    P, r = G.optimize(np.array(chain), edges[:9], 0, 5)
    assert np.abs(P - np.array(chain)).max() < 1e-9 and r["chi2_final"] <= r["chi2_initial"]


# ---- the rejected-trial path: what tests/graph_cases.py holds, decided by the restatement alone -------------------------------
def _runs(c):
    return GC.reference(c.name, c.iterations, "direct"), GC.reference(c.name, c.iterations, "pcg")


def test_trace_has_one_entry_per_trial_and_changes_nothing_else():
    from aria_slam_amd import graph_ref as G
    c = GC.BY_NAME["separate104"]
    poses, edges = GC.graph(c.name)
    P, r = G.optimize(poses, edges, c.fixed, c.iterations, "pcg")
    tr = r["trace"]
    assert len(tr) == r["trials"] and sum(t["accepted"] for t in tr) == r["iterations_done"]
    assert sum(t["solver_iterations"] for t in tr) == r["pcg_iterations"]
    assert all(set(t) == {"iteration", "trial", "rho", "accepted", "lambda_", "chi2_new", "solver_iterations"} for t in tr)
    assert [t["chi2_new"] for t in tr if t["accepted"]] == r["chi2_history"]
    # the iteration counts up at every accept, the trial restarts at 0; lambda before a trial follows the header's rule
    it, trial, ni = 0, 0, 2.0
    for a, b in zip(tr, tr[1:] + [None]):
        assert (a["iteration"], a["trial"]) == (it, trial)
        if a["accepted"]:
            nxt, it, trial, ni = a["lambda_"] * GC.update_factor(a["rho"]), it + 1, 0, 2.0
        else:
            nxt, trial, ni = a["lambda_"] * ni, trial + 1, ni * 2
        assert nxt == (b["lambda_"] if b else r["lambda_"])
    # a shorter call is the beginning of a longer one
    _P, r2 = G.optimize(poses, edges, c.fixed, 2, "pcg")
    assert r2["trace"] == tr[:len(r2["trace"])] and r2["trace"][-1]["accepted"]


@pytest.mark.parametrize("name", [c.name for c in GC.CASES])
def test_rejected_trial_case_has_its_pattern_under_both_solvers_with_a_margin(name):
    """A condition on the inputs: no decision of a case is near enough to rho = 0 for another summation order to flip it."""
    from aria_slam_amd import graph_ref as G
    c = GC.BY_NAME[name]
    poses, edges = GC.graph(name)
    assert G.check_graph(len(poses), edges, c.fixed)
    (Pd, rd), (Pp, rp) = _runs(c)
    assert GC.pattern(rd) == GC.pattern(rp) == c.pattern
    rho_d, rho_p = (np.array([t["rho"] for t in r["trace"]]) for r in (rd, rp))
    for r, P in ((rd, Pd), (rp, Pp)):
        assert r["trials"] == len(c.pattern) and r["iterations_done"] == c.pattern.count("A") and r["valid"] == 1
        assert P[c.fixed].tobytes() == poses[c.fixed].tobytes()
    if name not in GC.EXEMPT:
        assert rd["iterations_done"] == c.iterations and rd["stop_reason"] == G.STOP_ITERATIONS
        lo = np.minimum(np.abs(rho_d), np.abs(rho_p))
        print(name, "min |rho| %.3g, min |rho| / |rho_direct - rho_pcg| %.3g" % (lo.min(), (lo / np.abs(rho_d - rho_p)).min()))
        assert (lo >= GC.RHO_MIN).all(), lo.min()
        assert (lo >= GC.RHO_MARGIN * np.abs(rho_d - rho_p)).all()
        # the copied figures are this table's: one entry per k, the smallest |rho| as recorded, and every gap of every k
        # within a factor of two of its record. On the build the table was measured on they agree to the three digits
        # printed; the band is for another NumPy / SciPy build, where a PCG solve may stop one iteration earlier or later
        # and move a gap by the ratio of two consecutive residuals. The device's allowance is ten times the record.
        assert len(GC.GAPS[name]) == c.iterations and abs(GC.MIN_RHO[name] - lo.min()) <= 1e-3
        for k in range(1, c.iterations + 1):
            for got, want in zip(GC.gap(name, k), GC.GAPS[name][k - 1]):
                assert 0.5 * want <= got <= 2 * want, (k, GC.gap(name, k), GC.GAPS[name][k - 1])
        return
    assert name not in GC.GAPS
    for r, P in ((rd, Pd), (rp, Pp)):
        assert (r["iterations_done"], r["trials"], r["stop_reason"]) == (0, G.MAX_TRIALS, G.STOP_TRIALS)
        assert P.tobytes() == poses.tobytes()
    if name == "exact":                      # exempt: rho is exactly 0, the case that tells rho > 0 from rho >= 0
        assert not rho_d.any() and not rho_p.any()
        lam0 = 1e-5 * max(G.linearize(poses, edges)[2][v, k, k] for v in range(1, len(poses)) for k in range(6))
        for r in (rd, rp):
            assert r["chi2_initial"] == r["chi2_final"] == 0.0 and r["pcg_iterations"] == 0
            assert r["lambda_"] == lam0 * 2.0 ** 55 == 3963167672086.0366
            assert [t["lambda_"] for t in r["trace"]] == [lam0 * 2.0 ** (k * (k + 1) // 2) for k in range(10)]
    else:                                    # exempt: rho is not finite, the trial the finiteness guard is there for
        assert name == "overflow" and all(np.isfinite(e[2]) for e in edges)
        assert not np.isfinite(rho_d).any() and not np.isfinite(rho_p).any()
        for r in (rd, rp):
            assert not any(np.isfinite(t["chi2_new"]) for t in r["trace"]) and not np.isfinite(r["chi2_initial"])


def test_the_table_covers_the_rejected_trial_path():
    from aria_slam_amd import graph_ref as G
    src = open(os.path.join(ROOT, "aria_slam_amd", "csrc", "graph_optimize.hip")).read()
    lanes = int(re.search(r"GRAPH_BLOCK\s*=\s*(\d+)", src).group(1))
    shared = open(os.path.join(ROOT, "aria_slam_amd", "csrc", "solver_device.h")).read()      # the trial cap of both LM kernels
    assert "trial < LM_MAX_TRIALS" in src
    assert lanes == 512 and int(re.search(r"LM_MAX_TRIALS\s*=\s*(\d+)", shared).group(1)) == G.MAX_TRIALS == 10
    on_chip_edges = 544                      # the on-chip form of the one-vertex-per-lane solver holds this many
    seen = set()
    for c in GC.CASES:
        poses, edges = GC.graph(c.name)
        tr = GC.reference(c.name, c.iterations, "pcg")[1]["trace"]
        rejecting = sorted({t["iteration"] for t in tr if not t["accepted"]})
        accepts = c.pattern.count("A")
        if c.name in GC.EXEMPT:
            seen.add("exact minimum" if all(t["rho"] == 0.0 for t in tr) else "overflow")
            continue
        assert GC.pattern({"trace": tr}) == c.pattern
        if c.pattern.count("r") == 1:
            seen.add("one rejection, first iteration" if rejecting == [0] else "one rejection, later iteration")
        if "rrr" in c.pattern:
            seen.add("ni reaches 8")
        if len(rejecting) >= 2 and accepts > rejecting[-1]:      # every iteration ends in an accept: accepts lie between
            seen.add("separate iterations" if "separate iterations" not in seen else "separate iterations, twice")
        if rejecting and len(poses) <= lanes and len(edges) > on_chip_edges:
            assert c.handle and c.handle[0] <= lanes and c.handle[1] >= len(edges)
            seen.add("off-chip W")
        if rejecting and len(poses) > lanes:
            assert c.handle and c.handle[0] == 1024 and c.handle[1] >= len(edges)
            seen.add("strided solver")
        if rejecting and len(poses) <= lanes and len(edges) <= on_chip_edges:
            assert c.handle is None
            seen.add("on-chip W")
        if rejecting and c.fixed != 0:
            seen.add("fixed vertex")
        # the two ends of the update factor, each clear of its threshold by 0.05
        for t in tr:
            raw = 1.0 - (2.0 * t["rho"] - 1.0) ** 3
            if t["accepted"] and raw <= 1.0 / 3.0 - 0.05:
                assert t["rho"] > GC.CLAMP_RHO and GC.update_factor(t["rho"]) == 1.0 / 3.0
                seen.add("clamp")
            if t["accepted"] and raw >= 1.05:
                seen.add("lambda grows on an accept")
    want = {"one rejection, first iteration", "one rejection, later iteration", "ni reaches 8", "separate iterations",
            "separate iterations, twice", "off-chip W", "strided solver", "on-chip W", "fixed vertex", "clamp",
            "lambda grows on an accept", "exact minimum", "overflow"}
    assert seen == want, want ^ seen
    # the trials the table's notes name (there counted from 1): "clamp" trial 2, "first" trial 2, "three" trial 4
    rho = lambda name, k: GC.reference(name, GC.BY_NAME[name].iterations, "pcg")[1]["trace"][k]["rho"]
    assert GC.update_factor(rho("clamp", 1)) == 1.0 / 3.0 < min(GC.update_factor(rho("clamp", 0)), GC.update_factor(rho("clamp", 2)))
    assert GC.update_factor(rho("first", 1)) > 1.05 and GC.update_factor(rho("three", 3)) > 1.05


# ---- the reference class's bookkeeping ---------------------------------------------------------------------------------------
def test_bookkeeping_of_the_reference_class():
    from aria_slam_amd import graph_ref as G
    rng = np.random.default_rng(5)
    T = {k: G.random_pose(rng) for k in (7, 3, 5, 9)}
    g = G.PoseGraphOptimizer()
    assert np.array_equal(g.get_optimized_pose(1), np.eye(4)) and g.get_all_poses() == []
    g.optimize(3)                                               # an empty graph: nothing happens
    for k in (7, 3, 5):                                         # first ADDED is 7, not the smallest id
        g.set_initial_pose(k, T[k])
    assert g.index == {7: 0, 3: 1, 5: 2}
    assert g.add_odometry_edge(7, 3, G.inv(T[7]) @ T[3] @ G.random_pose(rng, 0.05, 0.05))
    assert g.add_loop_edge(3, 5, G.inv(T[3]) @ T[5] @ G.random_pose(rng, 0.05, 0.05), 2.0)
    assert not g.add_odometry_edge(5, 9, np.eye(4))             # 9 unknown: dropped silently
    assert not g.add_loop_edge(4, 7, np.eye(4))
    assert len(g.edges) == 2 and g.edges[0][2] == 1.0 and g.edges[1][2] == 20.0      # loop edges at 10x
    assert np.array_equal(g.get_optimized_pose(9), np.eye(4))   # unknown id: identity
    g.set_initial_pose(5, T[9])                                 # known id: the estimate is overwritten, no new vertex
    assert len(g.poses) == 3 and np.array_equal(g.get_optimized_pose(5), T[9])
    allp = g.get_all_poses()                                    # ascending id order: 3, 5, 7
    assert [p.tobytes() for p in allp] == [g.get_optimized_pose(k).tobytes() for k in (3, 5, 7)]
    g.optimize(5)
    assert g.get_optimized_pose(7).tobytes() == T[7].tobytes()  # the fixed vertex is the first added
    assert g.last_result["chi2_final"] < g.last_result["chi2_initial"]
    assert not np.array_equal(g.get_optimized_pose(3), T[3])
    g.clear()
    assert g.get_all_poses() == [] and g.edges == [] and np.array_equal(g.get_optimized_pose(7), np.eye(4))


# ---- the kernel's listing and the builds ---------------------------------------------------------------------------------------
def _listing():
    csrc = os.path.join(ROOT, "aria_slam_amd", "csrc")
    out = os.path.join(ROOT, "build", "isa")
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, "graph_optimize.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                           "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-fast-math", "-I" + os.path.join(ROOT, "include"),
                           "-I" + csrc, "--cuda-device-only", "-S", "-w", "-o", path, os.path.join(csrc, "graph_optimize.hip")])
    return open(path).read()


def test_graph_kernel_cross_compiles_without_scratch():
    """The PCG loop lives in k_graph_lm (one persistent workgroup per graph): the whole kernel has no scratch."""
    text = _listing()
    body, meta = S.kernel_body(text, "k_graph_lm")
    assert len(body) > 500
    assert meta.get("ScratchSize", -1) == 0, meta
    in_loop, outside = S.scratch_accesses(text, "k_graph_lm")
    assert not in_loop and not outside
    assert meta.get("LDSByteSize", 0) <= 64 * 1024


def test_graph_optimize_is_in_the_product_build_and_has_no_float_atomics():
    mk = open(os.path.join(ROOT, "aria_slam_amd", "csrc", "Makefile")).read()
    src_line = [ln for ln in mk.splitlines() if ln.startswith("SRC :=")][0]
    assert "graph_optimize.hip" in src_line
    src = open(os.path.join(ROOT, "aria_slam_amd", "csrc", "graph_optimize.hip")).read()
    # the rules below follow the code into the shared headers this file includes
    src += "".join(open(os.path.join(ROOT, "aria_slam_amd", "csrc", h)).read() for h in ("stage_handle.h", "ransac_device.h", "solver_device.h", "graph_lm_device.h") if '#include "%s"' % h in src)
    assert '#include "graph_lm_device.h"' in src      # the adjacency build and the solver live there
    assert "getenv" not in src
    # the only atomics are the integer ones of the adjacency build (counts and fill cursors) and the error word
    atomics = re.findall(r"atomic\w+\(&?\s*([\w.\[\]>-]+)", src)
    assert atomics and all(a.startswith(("S.aoff", "S.cur", "err")) for a in atomics), atomics
    # no grid-wide synchronisation: one workgroup per graph
    assert "cooperative" not in src and "grid.sync" not in src and "hipLaunchCooperativeKernel" not in src


def test_host_adapters_build_with_the_pose_graph_optimizer(aria):
    pkg = os.path.join(ROOT, "aria_slam_amd")
    subprocess.check_call(["make", "-C", os.path.join(pkg, "host"), "-s"])
    syms = subprocess.run(["nm", "-DC", os.path.join(pkg, "libaria_hip_adapters.so")], capture_output=True, text=True,
                          check=True).stdout
    for m in ("setInitialPose", "addOdometryEdge", "addLoopEdge", "optimize", "getOptimizedPose", "getAllPoses", "clear"):
        assert "aria::adapters::hip::HipPoseGraphOptimizer::" + m in syms, m
    exe = os.path.join(pkg, "euroc_frontend")
    usage = subprocess.run([exe], capture_output=True, text=True)
    assert "--optimize" in usage.stderr and "not reproduced" in usage.stderr
    # the selftest driver compiles against the adapter
    out = os.path.join(ROOT, "build", "graph_selftest")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(pkg, "host", "include"),
                           os.path.join(ROOT, "tests", "cpp", "graph_selftest.cpp"), "-o", out, "-L" + pkg, "-laria_hip_adapters",
                           "-laria_orb_hip", "-lz", "-Wl,-rpath," + pkg])
