"""Loop alignment (include/aria_orb_hip.h, "loop alignment"): the parts that need no GPU -- exports, record layouts, the
refusals of create, the NumPy restatement (aria_slam_amd/sim3_ref.py) against ground truth and against itself, the
association rule against a brute-force join, what the case table of tests/sim3_cases.py covers, and the kernels' listing."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import isa_kernel_stats as S   # noqa: E402
import sim3_cases as SC   # noqa: E402

SIM3_SYMBOLS = ["aria_sim3_default_config", "aria_sim3_create", "aria_sim3_destroy", "aria_sim3_stream", "aria_sim3_check",
                "aria_sim3_estimate", "aria_sim3_estimate_batch_device", "aria_sim3_debug_hypotheses",
                "aria_sim3_associate_batch_device"]
KERNELS = ("k_sim3_stage", "k_sim3_hyp", "k_sim3_score", "k_sim3_finish", "k_sim3_assoc_scatter", "k_sim3_assoc_gather")

# The cases of the table that are not exact-set, by index: the cap is 3, and none is an edge case.
NOT_EXACT = [9, 32]


def test_sim3_symbols_exported_and_listed(aria):
    from aria_slam_amd import _lib
    L = aria.load_library()
    header = open(os.path.join(ROOT, "include", "aria_orb_hip.h")).read()
    for name in SIM3_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), "%s not declared in the header" % name
        assert hasattr(L, name), "libaria_orb_hip.so does not export %s" % name
        assert name in _lib.EXPORTS, "%s missing from _lib.EXPORTS" % name
    assert aria.abi_version() == 4
    assert aria.HipSim3Aligner.__name__ in aria.__all__


def test_sim3_record_layouts_and_defaults(aria):
    from aria_slam_amd import _lib
    assert _lib.SIM3_CORR_DTYPE.itemsize == 64             # double X1[3], X2[3], float u1, v1, u2, v2
    assert _lib.SIM3_RESULT_DTYPE.itemsize == 136          # double R[9], t[3], s, rms_px + 6 ints
    assert C.sizeof(_lib.Sim3Config) == 96
    cfg = _lib.Sim3Config()
    aria.load_library().aria_sim3_default_config(C.byref(cfg))
    assert cfg.struct_size == 96 and cfg.hypotheses == 1024 and cfg.threshold_px == 3.0 and cfg.refine_iters == 5
    assert cfg.fix_scale == 0 and cfg.reserved == 0 and (cfg.min_scale, cfg.max_scale) == (0.05, 20.0) and not cfg.stream
    assert (cfg.fx, cfg.fy, cfg.cx, cfg.cy) == (458.654, 457.296, 367.215, 248.375) and cfg.seed == 0
    assert (SC.MIN_SCALE, SC.MAX_SCALE) == (cfg.min_scale, cfg.max_scale)
    src = open(os.path.join(ROOT, "aria_slam_amd", "csrc", "sim3_align.hip")).read()
    assert re.search(r"SIM3_TILE = (\d+);", src).group(1) == str(SC.TILE)


@pytest.mark.parametrize("field,value", [("struct_size", 0), ("hypotheses", 0), ("hypotheses", 100), ("hypotheses", 16448),
                                         ("refine_iters", -1), ("refine_iters", 17), ("fix_scale", 2), ("fix_scale", -1),
                                         ("fx", 0.0), ("fy", -1.0), ("cx", float("nan")), ("cy", float("inf")),
                                         ("threshold_px", 0.0), ("threshold_px", float("nan")), ("min_scale", 0.0),
                                         ("min_scale", float("nan")), ("max_scale", 0.01), ("max_scale", float("inf"))])
def test_sim3_create_refuses_a_bad_config_before_touching_a_device(aria, field, value):
    from aria_slam_amd import _lib
    L = aria.load_library()
    cfg = _lib.Sim3Config()
    L.aria_sim3_default_config(C.byref(cfg))
    setattr(cfg, field, value)
    h = C.c_void_p()
    assert L.aria_sim3_create(C.byref(cfg), C.byref(h)) == -1 and not h      # ARIA_E_INVALID
    assert L.aria_sim3_check(None) == -1 and L.aria_sim3_stream(None) is None
    L.aria_sim3_destroy(None)


def test_sampler_is_the_pose_stage_hash_with_three_slots():
    from aria_slam_amd import pose_ref as P
    from aria_slam_amd import sim3_ref as N
    for seed, pair, n in ((0, 0, 100), (3, 1000000, 600), (SC.HIGH_SEED, 5, 3)):
        idx = N.sample_indices(seed, pair, 64, n)
        assert idx.shape == (64, 3) and np.array_equal(idx, P.sample_indices(seed, pair, 64, n, k=3))
        assert (np.sort(idx, axis=1)[:, 1:] != np.sort(idx, axis=1)[:, :-1]).all() and idx.min() >= 0 and idx.max() < n
    assert (N.sample_indices(0, 0, 64, 2) == -1).all()      # n < 3: no sample


@pytest.mark.parametrize("k", range(4))
@pytest.mark.parametrize("s", [0.25, 1.0, 4.0])
def test_closed_form_recovers_exact_similarities(k, s):
    """Exact point pairs: every valid three-point sample gives the similarity, to rounding; with fix_scale the same on a
    metric scene. The rotation is proper (det +1) although three points only span a plane."""
    from aria_slam_amd import sim3_ref as N
    R, t = SC.motion(k)
    rng = np.random.default_rng(10 + k)
    X1 = rng.uniform(-3, 3, (64, 3, 3)) + [0, 0, 8]
    X2 = s * (X1 @ R.T) + s * t
    Rh, th, sh, ok = N.solve_minimal(X1, X2)
    assert ok.all()
    assert np.abs(Rh - R).max() < 1e-9 and np.abs(th - s * t).max() < 1e-8 * s and np.abs(sh / s - 1).max() < 1e-10
    assert np.abs(np.linalg.det(Rh) - 1.0).max() < 1e-9       # of the order of the entries' error
    if s == 1.0:
        Rf, tf, sf, okf = N.solve_minimal(X1, X2, fix_scale=1)
        assert okf.all() and (sf == 1.0).all() and np.abs(Rf - R).max() < 1e-9 and np.abs(tf - t).max() < 1e-8
    # the Jacobi of the restatement is the device's fixed ten sweeps: it diagonalises to rounding
    G = rng.normal(size=(16, 3, 3))
    G = G @ G.transpose(0, 2, 1)
    lam, V = N.jacobi3(G)
    assert np.abs(np.sort(lam, axis=1) - np.linalg.eigvalsh(G)).max() < 1e-12 * np.abs(lam).max()
    assert np.abs(V.transpose(0, 2, 1) @ V - np.eye(3)).max() < 1e-14


def test_sample_validity_rules():
    from aria_slam_amd import sim3_ref as N
    a, b = np.array([0.0, 0.0, 5.0]), np.array([1.0, 0.5, 6.0])
    tri = np.stack([a, b, np.array([0.3, -1.0, 7.0])])[None]
    line = np.stack([a, b, a + 0.4 * (b - a)])[None]
    twice = np.stack([a, b, a])[None]
    assert N.solve_minimal(tri, 2.0 * tri + 1.0)[3].all()
    for bad in (line, twice):
        assert not N.solve_minimal(bad, tri)[3].any() and not N.solve_minimal(tri, bad)[3].any()   # either frame
    # the bounds on s
    assert N.solve_minimal(tri, 0.06 * tri)[3].all() and N.solve_minimal(tri, 19.0 * tri)[3].all()
    assert not N.solve_minimal(tri, 0.01 * tri)[3].any() and not N.solve_minimal(tri, 30.0 * tri)[3].any()
    assert N.solve_minimal(tri, 30.0 * tri, fix_scale=1)[3].all()                                    # no scale, no bound
    R, t, s, ok = N.solve_minimal(tri, np.full_like(tri, np.inf))
    assert not ok.any() and not R.any() and not t.any() and not s.any()                            # the model is not finite


def test_exp_series_is_exp_near_zero_and_has_no_libm():
    from aria_slam_amd import sim3_ref as N
    for x in (-0.5, -1e-3, 0.0, 1e-9, 0.02, 0.5):           # the remainder at 0.5: 0.5^13 / 13! = 2e-14
        assert abs(N.exp_series(x) - np.exp(x)) < 1e-13
    assert N.exp_series(0.0) == 1.0 and N.exp_series(-30.0) > 20.0      # far out the polynomial is not exp: the bounds on s catch it
    src = open(os.path.join(ROOT, "aria_slam_amd", "csrc", "sim3_align.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert not re.search(r"\bexp\s*\(", code) and not re.search(r"\bpow\s*\(", code)


def test_gauss_newton_jacobian_agrees_with_central_differences():
    from aria_slam_amd import sim3_ref as N
    rng = np.random.default_rng(5)
    R = N.rot([0.2, -1.0, 0.4], 13.0)
    t, s = np.array([0.6, -0.2, 0.4]), 1.7
    X1 = rng.uniform(-2, 2, (20, 3)) + [0, 0, 7]
    X2 = s * (X1 @ R.T) + t + rng.normal(0, 0.05, (20, 3))
    x1, x2 = rng.uniform(-0.5, 0.5, (20, 2)), rng.uniform(-0.5, 0.5, (20, 2))
    J = N.gn_jacobian(R, t, s, X1, X2)
    eps = 1e-6
    for k in range(7):
        e = np.zeros(7)
        e[k] = eps
        out = []
        for sign in (1.0, -1.0):
            d = sign * e
            E, es = N.exp_so3(d[:3]), N.exp_series(d[6])
            out.append(N.residuals(E @ R, es * (E @ t) + d[3:6], es * s, X1, X2, x1, x2))
        assert np.abs((out[0] - out[1]) / (2 * eps) - J[:, :, k]).max() < 1e-7, k
    assert not J[:, :2, 6].any()                            # sigma moves Y2 along its ray: no image motion in camera 2
    # and steps from a perturbed model land on the model the residuals vanish at
    proj = lambda X: X[:, :2] / X[:, 2:]   # noqa: E731
    X2e, X2m = s * (X1 @ R.T) + t, (X1 @ R.T) + t
    Rp = N.exp_so3([0.01, -0.02, 0.015]) @ R
    R2, t2, s2, steps = N.refine(Rp, t + [0.05, -0.03, 0.1], s * 1.05, X1, X2e, proj(X1), proj(X2e), 10)
    assert steps <= 10 and np.abs(R2 - R).max() < 1e-10 and np.abs(t2 - t).max() < 1e-9 and abs(s2 - s) < 1e-9
    R3, t3, s3, _ = N.refine(Rp, t + [0.05, -0.03, 0.1], 1.0, X1, X2m, proj(X1), proj(X2m), 10, fix_scale=1)
    assert s3 == 1.0 and np.abs(R3 - R).max() < 1e-10 and np.abs(t3 - t).max() < 1e-9


def test_refinement_ends_where_the_scale_cannot_be_seen_or_leaves_its_bounds():
    from aria_slam_amd import sim3_ref as N
    rng = np.random.default_rng(6)
    X1 = rng.uniform(-2, 2, (30, 3)) + [0, 0, 7]
    R = N.rot([0, 1, 0], 5.0)
    x1 = X1[:, :2] / X1[:, 2:]
    # two cameras at one centre: the sigma column is zero, the pivot is not positive, no step is taken
    X2 = 2.0 * (X1 @ R.T)
    x2 = X2[:, :2] / X2[:, 2:]
    Rr, tr, sr, steps = N.refine(R, np.zeros(3), 2.0, X1, X2, x1, x2, 5)
    assert steps == 0 and sr == 2.0 and np.array_equal(Rr, R)
    # a step that would take s beyond max_scale is not taken
    t = np.array([0.5, 0.0, 0.2])
    X2 = 2.0 * (X1 @ R.T) + t
    x2 = X2[:, :2] / X2[:, 2:]
    _, _, sr, steps = N.refine(R, t, 1.9, X1, X2, x1, x2, 5, max_scale=1.95)
    assert steps == 0 and sr == 1.9
    assert N.refine(R, t, 1.9, X1, X2, x1, x2, 5)[3] >= 1


def _brute_force_join(pts, a1, a2, v1, v2, T1, T2, k1, k2, m, kp_stride):
    out, back = [], []
    for i in range(len(m)):
        q, tr = int(m["query_idx"][i]), int(m["train_idx"][i])
        pos = []
        for anchor, view, key in ((a1, v1, q), (a2, v2, tr)):
            hit = [j for j in range(len(pts)) if pts["pair"][j] == anchor and pts["idx%d" % view][j] == key and 0 <= key < kp_stride]
            pos.append(min(hit) if hit else None)
        if pos[0] is None or pos[1] is None:
            continue
        out.append((T1[:, :3] @ pts["X"][pos[0]] + T1[:, 3], T2[:, :3] @ pts["X"][pos[1]] + T2[:, 3],
                    k1["x"][q], k1["y"][q], k2["x"][tr], k2["y"][tr]))
        back.append(i)
    return out, back


def test_association_rule_against_a_brute_force_join():
    """A small arena with duplicates (the lowest arena position wins, per side), points missing on either side, points of
    other pairs, and arena indices outside [0, kp_stride) that own nothing."""
    from aria_slam_amd import _lib
    from aria_slam_amd import sim3_ref as N
    rng = np.random.default_rng(8)
    n_pts, stride = 60, 12
    pts = np.zeros(n_pts, _lib.MAP_POINT_DTYPE)
    pts["pair"] = rng.choice([4, 5, 9], n_pts)
    pts["idx1"] = rng.integers(-2, stride + 3, n_pts)        # some out of range, many duplicates
    pts["idx2"] = rng.integers(-2, stride + 3, n_pts)
    pts["X"] = rng.uniform(-5, 5, (n_pts, 3)) + [1000.0, -2000.0, 500.0]        # a map far from the origin
    k1, k2 = np.zeros(stride, _lib.KP_DTYPE), np.zeros(stride, _lib.KP_DTYPE)
    k1["x"], k1["y"] = rng.uniform(0, 700, stride), rng.uniform(0, 400, stride)
    k2["x"], k2["y"] = rng.uniform(0, 700, stride), rng.uniform(0, 400, stride)
    m = np.zeros(40, _lib.MATCH_DTYPE)
    m["query_idx"], m["train_idx"] = rng.integers(0, stride, 40), rng.integers(0, stride, 40)
    centre = np.array([1000.0, -2000.0, 500.0])
    R1, R2 = N.rot([0, 1, 0], 20), N.rot([1, 0, 0.3], -10)
    T1 = np.concatenate([R1, (-R1 @ centre + [0.0, 0.0, 8.0])[:, None]], axis=1)     # the cameras look at the cloud
    T2 = np.concatenate([R2, (-R2 @ centre + [1.0, 0.0, 9.0])[:, None]], axis=1)
    total = 0
    for a1, a2, v1, v2 in ((5, 9, 1, 2), (5, 5, 2, 1), (4, 5, 2, 2), (9, 4, 1, 1), (5, 7, 1, 2)):
        corr, back = N.associate(pts, a1, a2, v1, v2, T1.ravel(), T2.ravel(), k1, k2, m, kp_stride=stride)
        want, wback = _brute_force_join(pts, a1, a2, v1, v2, T1, T2, k1, k2, m, stride)
        assert back.tolist() == wback and len(corr) == len(want)
        for c, w in zip(corr, want):
            assert np.abs(c["X1"] - w[0]).max() < 1e-9 and np.abs(c["X2"] - w[1]).max() < 1e-9      # another association of the sum
            assert (c["u1"], c["v1"], c["u2"], c["v2"]) == w[2:]
        total += len(corr)
        if a2 == 7:
            assert len(corr) == 0                              # keyframe 2 owns nothing
    assert total > 20
    # duplicates exist on both sides, and the camera coordinates are near the origin although the map is not
    own = pts[(pts["pair"] == 5) & (pts["idx1"] >= 0) & (pts["idx1"] < stride)]
    assert len(np.unique(own["idx1"])) < len(own)
    corr, _ = N.associate(pts, 5, 9, 1, 2, T1.ravel(), T2.ravel(), k1, k2, m, kp_stride=stride)
    assert np.abs(corr["X1"]).max() < 50 and np.abs(pts["X"]).max() > 1000


@pytest.mark.parametrize("case", SC.SIM3_CASES + SC.SIM3_BATCH, ids=SC.case_id)
def test_table_case_can_be_decided(case):
    """Conditions on the inputs, not measurements: a case that violates one is replaced, the condition stays."""
    rep = SC.report(case)
    ref, ext = rep["ref"], rep["ext"]
    assert rep["unambiguous"]                                  # no other hypothesis within the in-band points of the winner
    for k in ("valid", "best_hypothesis", "iterations", "refined", "n_inliers", "n_corr"):
        assert ext[k] == ref[k]                                # the extended run takes every decision the fp64 run takes
    assert np.array_equal(ext["mask"], ref["mask"])
    if not ref["valid"]:
        return
    for k in ("R", "t", "s", "rms_px"):
        assert np.isfinite(np.asarray(ref[k], np.float64)).all()
    assert SC.MIN_SCALE <= float(ref["s"]) <= SC.MAX_SCALE and abs(np.linalg.det(np.asarray(ref["R"], np.float64)) - 1.0) < 1e-9
    if not rep["exact"]:
        # a point of the winner's own band would change the refinement's input; and `refined` must not hang on the band
        assert rep["band_winner"] == 0
        assert ref["refit"] is None or abs(ref["n_refit"] - ref["n_winner"]) > rep["in_band"]


def test_table_covers_the_stage():
    reps = [SC.report(c) for c in SC.SIM3_CASES]
    cases = SC.SIM3_CASES
    T = SC.TILE
    assert {0, 2, 3, 4, 7, 40, 150, 600, T - 1, T, T + 1, 4096} <= {c.n for c in cases} and max(c.n for c in cases) == 4096
    assert {64, 320, 1024, 4096} <= {c.H for c in cases} and max(c.H for c in cases) == 4096
    assert {0, 3, SC.HIGH_SEED} <= {c.seed for c in cases} and SC.HIGH_SEED >> 63 == 1
    assert {0, 5, 1000000} <= {c.pair_base for c in cases}
    assert {0.25, 1.0, 4.0} <= {c.s for c in cases} and {0.0, 0.05, 0.5} <= {c.noise_px for c in cases}
    assert min(c.outliers for c in cases) == 0.0 and max(c.outliers for c in cases) == 0.5
    assert {0, 1} == {c.fix_scale for c in cases} and any(c.refine_iters == 0 for c in cases)
    assert {SC.EUROC, SC.LOOP} <= {c.K for c in cases}
    assert [c.n for c in SC.SIM3_BATCH] == [300, 0, T - 1, 2, T, 3, T + 1, 40, 600, 1, 150]
    # the exact-set condition is a cap: at most 3 cases with a correspondence inside the band, listed, none an edge case
    assert [i for i, r in enumerate(reps) if not r["exact"]] == NOT_EXACT == SC.NOT_EXACT and len(NOT_EXACT) <= 3
    assert not set(NOT_EXACT) & set(SC.EDGE_CASES)
    assert all(SC.report(c)["exact"] for c in SC.SIM3_BATCH)
    by = lambda f: [r for r in reps if f(r["case"])]   # noqa: E731
    # below a sample: invalid; exactly a sample: valid, no refinement; four: the least a refinement takes
    for r in by(lambda c: c.n < 3):
        assert r["ref"]["valid"] == 0 and r["ref"]["n_corr"] == r["case"].n
    three, four = by(lambda c: c.n == 3)[0]["ref"], by(lambda c: c.n == 4)[0]["ref"]
    assert three["valid"] == 1 and three["iterations"] == 0 and four["valid"] == 1 and four["n_winner"] == 4 and four["iterations"] > 0
    # refined where a refinement ran, except where the table says the winner was kept; both outcomes occur
    valid = [r for r in reps if r["ref"]["valid"]]
    assert any(r["ref"]["refined"] for r in valid) and any(r["ref"]["iterations"] and not r["ref"]["refined"] for r in valid)
    assert all(r["ref"]["iterations"] == 0 and r["ref"]["refined"] == 0 for r in valid if r["case"].refine_iters == 0)
    # the collinear cloud and the all-equal list: enough correspondences, every sample drawn, every one refused as degenerate
    for r in by(lambda c: c.shape == "line" or c.copies == 1.0):
        idx, counts = r["hyp"][0], r["hyp"][4]
        assert r["ref"]["valid"] == 0 and r["case"].n >= 3 and (idx >= 0).all() and (counts == -1).all()
    # the planar cloud is valid and refined: a plane is no degeneracy here
    planar = by(lambda c: c.shape == "planar")[0]["ref"]
    assert planar["valid"] == 1 and planar["refined"] == 1 and planar["n_inliers"] > 100
    # tie scenes: every valid hypothesis counts all n, the winner is the first of them and not hypothesis 0
    ties = [r for r in valid if r["case"].noise_px == 0.0 and 0 < r["case"].copies < 1]
    assert len(ties) == 2
    for r in ties:
        counts, best = r["hyp"][4], r["ref"]["best_hypothesis"]
        assert best >= 1 and counts.max() == r["case"].n == r["ref"]["n_winner"]
        assert (counts[best + 1:] == r["case"].n).sum() >= 1 and (counts[:best] < 0).all()
    # a true s beyond max_scale: the samples are drawn and refused by the bound
    far = by(lambda c: c.s > SC.MAX_SCALE)[0]
    assert far["ref"]["valid"] == 0 and (far["hyp"][0] >= 0).all() and (far["hyp"][4] == -1).all()
    assert far["case"]._replace(s=4.0) != far["case"] and SC.report(far["case"]._replace(s=4.0))["ref"]["valid"] == 1
    # fix_scale on a scene with s = 1.3: a model, few inliers; on a metric scene: the inliers
    off, metric = by(lambda c: c.fix_scale and c.s != 1.0)[0]["ref"], by(lambda c: c.fix_scale and c.s == 1.0)[0]["ref"]
    assert off["valid"] == 1 and off["n_inliers"] < 10 and float(off["s"]) == 1.0
    assert metric["valid"] == 1 and metric["n_inliers"] > 100 and float(metric["s"]) == 1.0
    # landmarks behind camera 2 on their pixels' rays: none is an inlier, the rest carry the model
    behind = by(lambda c: c.behind > 0)[0]
    k = int(round(behind["case"].n * behind["case"].behind))
    assert k == 45 and not behind["ref"]["mask"][1:1 + k].any() and behind["ref"]["n_inliers"] > 90
    # one coordinate that is not finite: the pair is refused before it is read
    nf = by(lambda c: c.nonfinite >= 0)[0]
    assert not nf["staged"]["finite"] and nf["ref"]["valid"] == 0 and nf["ref"]["n_corr"] == 0 and (nf["hyp"][4] == -1).all()


def test_ground_truth_cases_recover_the_similarity():
    """The worst error of the restatement over SC.GT_CASES, as tools/sim3_gap.py prints it: the numbers the GPU test doubles."""
    worst = [0.0, 0.0, 0.0, 1.0]
    for i in SC.GT_CASES:
        rep = SC.report(SC.SIM3_CASES[i])
        assert rep["ref"]["valid"] == 1, i
        r, t, s, prec = SC.truth_error(rep["ref"], rep)
        worst = [max(worst[0], r), max(worst[1], t), max(worst[2], s), min(worst[3], prec)]
    assert len(SC.GT_CASES) >= 15
    assert abs(worst[0] - 0.1034) < 1e-3 and abs(worst[1] - 0.01361) < 1e-4 and abs(worst[2] - 0.00588) < 1e-4 and worst[3] == 1.0


def _listing():
    csrc = os.path.join(ROOT, "aria_slam_amd", "csrc")
    out = os.path.join(ROOT, "build", "isa")
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, "sim3_align.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                           "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-fast-math", "-I" + os.path.join(ROOT, "include"),
                           "-I" + csrc, "--cuda-device-only", "-S", "-w", "-o", path, os.path.join(csrc, "sim3_align.hip")])
    return open(path).read()


def test_sim3_kernels_cross_compile_without_scratch():
    text = _listing()
    for k in KERNELS:
        body, meta = S.kernel_body(text, k)
        assert len(body) > 20, k
        assert meta.get("ScratchSize", -1) == 0, (k, meta)
        in_loop, outside = S.scratch_accesses(text, k)
        assert not in_loop and not outside, k
    _, meta = S.kernel_body(text, "k_sim3_score")
    assert meta.get("LDSByteSize", 0) == SC.TILE * 40 <= 160 * 1024       # ten floats per correspondence


def test_sim3_align_is_in_the_product_build_and_reads_no_environment():
    mk = open(os.path.join(ROOT, "aria_slam_amd", "csrc", "Makefile")).read()
    src_line = [ln for ln in mk.splitlines() if ln.startswith("SRC :=")][0]
    assert "sim3_align.hip" in src_line
    src = open(os.path.join(ROOT, "aria_slam_amd", "csrc", "sim3_align.hip")).read()
    assert "getenv" not in src
    assert "atomicAdd(float" not in src and "atomicAdd(double" not in src
