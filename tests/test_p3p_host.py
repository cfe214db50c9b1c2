"""The P3P minimal solver of the absolute pose stage (include/aria_orb_hip.h, "Minimal solver, P3P"): the parts that need no
GPU -- exports, the unchanged record layouts, the NumPy restatement (aria_slam_amd/pnp_ref.py, solver="p3p") against ground
truth and against itself, what the case table of tests/p3p_cases.py covers, and the new kernel's listing."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import isa_kernel_stats as S   # noqa: E402
import p3p_cases as QC   # noqa: E402
import pnp_cases as PC   # noqa: E402

P3P_SYMBOLS = ["aria_pnp_set_solver", "aria_pnp_get_solver"]


def test_solver_symbols_exported_and_listed_and_the_abi_is_unchanged(aria):
    import ctypes as C
    from aria_slam_amd import _lib
    L = aria.load_library()
    header = open(os.path.join(ROOT, "include", "aria_orb_hip.h")).read()
    for name in P3P_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), "%s not declared in the header" % name
        assert hasattr(L, name), "libaria_orb_hip.so does not export %s" % name
        assert name in _lib.EXPORTS, "%s missing from _lib.EXPORTS" % name
    assert re.search(r"#define\s+ARIA_PNP_SOLVER_DLT6\s+0\b", header) and re.search(r"#define\s+ARIA_PNP_SOLVER_P3P\s+1\b", header)
    assert "Known limit" not in header[header.index("absolute pose from the point map"):header.index("local bundle adjustment")]
    assert aria.abi_version() == 4
    assert C.sizeof(_lib.PnpConfig) == 72
    cfg = _lib.PnpConfig()
    L.aria_pnp_default_config(C.byref(cfg))
    assert cfg.struct_size == 72 and cfg.hypotheses == 1024
    from aria_slam_amd import pnp
    assert pnp.SOLVERS == {"dlt": 0, "p3p": 1}


def test_sampler_is_the_pose_stage_hash_with_four_slots():
    from aria_slam_amd import pnp_ref as N
    from aria_slam_amd import pose_ref as P
    assert N.MIN_CORR_P3P == 4 and N.min_corr("p3p") == 4 and N.min_corr("dlt") == N.MIN_CORR == 6
    for seed, pair, n in ((0, 0, 100), (3, 1000000, 600), (PC.HIGH_SEED, 5, 4)):
        idx = N.sample_indices(seed, pair, 64, n, k=4)
        assert idx.shape == (64, 4) and np.array_equal(idx, P.sample_indices(seed, pair, 64, n, k=4))
        assert (np.sort(idx, axis=1)[:, 1:] != np.sort(idx, axis=1)[:, :-1]).all() and idx.min() >= 0 and idx.max() < n
        # the first four slots of the six-slot draw: one hash, two sample sizes
        if n >= 6:
            assert np.array_equal(idx, N.sample_indices(seed, pair, 64, n)[:, :4])
    assert (N.sample_indices(0, 0, 64, 3, k=4) == -1).all()      # n < 4: no sample
    corr = N.synth_pnp(1, 50, *PC.motion(1))[0]
    idx = N.hypotheses(corr, n_hyp=64, solver="p3p")[0]
    assert idx.shape == (64, 6) and (idx[:, 4:] == -1).all() and np.array_equal(idx[:, :4], N.sample_indices(0, 0, 64, 50, k=4))


def _exact_scene(seed, n, k, planar):
    """A synth_pnp scene whose world points are exact for their float pixels: each point keeps its depth and is moved onto
    its pixel's ray (as tests/test_pnp_host.py::test_pnp_ref_recovers_noise_free_poses does)."""
    from aria_slam_amd import pnp_ref as N
    R, t = PC.motion(k)
    corr, _truth, Rt, tt = N.synth_pnp(seed, n, R, t, 0.0, 0.0, planar=planar)
    fx, fy, cx, cy = N.EUROC_K
    Xc = corr["X"] @ Rt.T + tt
    z = Xc[:, 2]
    Xc = np.stack([(corr["u"].astype(np.float64) - cx) / fx * z, (corr["v"].astype(np.float64) - cy) / fy * z, z], axis=1)
    corr["X"] = (Xc - tt) @ Rt
    return corr, Rt, tt


@pytest.fixture(scope="module")
def noise_free():
    """The four motions, 3-D and planar, 500 four-samples each (the stage's own sampler with seed = the motion): the solver's
    output with its detail, shared by the tests below."""
    from aria_slam_amd import pnp_ref as N
    runs = []
    for planar in (False, True):
        for k in range(4):
            corr, Rt, tt = _exact_scene(40 + k, 100, k, planar)
            st = N.stage(corr)
            idx = N.sample_indices(k, 0, 500, 100, k=4)
            X, xy = st["X"][idx], st["xy"][idx]
            runs.append(dict(planar=planar, k=k, corr=corr, Rt=Rt, tt=tt, X=X, xy=xy, out=N.solve_p3p(X, xy, detail=True)))
    return runs


def test_p3p_recovers_noise_free_poses(noise_free):
    """Every sample yields a model; on the 3-D scenes every model is within 1e-9 of the truth, on the planar scenes at least
    99 % are within 1e-9 and all within 1e-5; the samples have 1 to 4 candidates; estimate(solver="p3p") recovers the pose to
    1e-9. Measured with this restatement: 3-D worst 4.1e-12; planar 99.6 % within 1e-9, 1999 of 2000 within 1e-7, worst
    2.4e-7."""
    from aria_slam_amd import pnp_ref as N
    err = {False: [], True: []}
    ncand = []
    for r in noise_free:
        R, t, ok, slot, info = r["out"]
        assert ok.all() and (slot >= 0).all() and (slot <= 3).all()
        assert (info["alive"][np.arange(500), slot]).all() and not info["degenerate"].any()
        err[r["planar"]].append(np.maximum(np.abs(R - r["Rt"]).reshape(500, -1).max(axis=1), np.abs(t - r["tt"]).max(axis=1)))
        ncand.append(info["alive"].sum(axis=1))
        e = N.estimate(r["corr"], n_hyp=64, solver="p3p")
        assert e["valid"] == 1 and e["n_inliers"] == 100 and e["mask"].all() and e["refined"] == 1
        assert np.abs(e["R"] - r["Rt"]).max() < 1e-9 and np.abs(e["t"] - r["tt"]).max() < 1e-9 and e["rms_px"] < 1e-6
    e3, ep, ncand = np.concatenate(err[False]), np.concatenate(err[True]), np.concatenate(ncand)
    print("3-D worst %.2e; planar within 1e-9: %.4f, within 1e-7: %d of %d, worst %.2e; candidates per sample %s" %
          (e3.max(), (ep < 1e-9).mean(), (ep < 1e-7).sum(), len(ep), ep.max(), np.bincount(ncand).tolist()))
    assert len(e3) == len(ep) == 2000
    assert e3.max() < 1e-9
    assert (ep < 1e-9).mean() >= 0.99 and ep.max() < 1e-5
    assert ncand.min() >= 1 and ncand.max() <= 4 and len(set(ncand.tolist())) >= 3


def test_polish_leaves_the_distance_equations_satisfied(noise_free):
    """Every candidate's three distance residuals after the polish are at most 1e-12 relative to max a_ij."""
    worst = 0.0
    for r in noise_free:
        info = r["out"][4]
        L = info["lengths"]
        a12, a13, a23 = (v[:, None] for v in info["a"])
        b12, b13, b23 = (v[:, None] for v in info["b"])
        l1, l2, l3 = L[:, :, 0], L[:, :, 1], L[:, :, 2]
        res = np.stack([l1 * l1 + l2 * l2 - 2 * b12 * l1 * l2 - a12, l1 * l1 + l3 * l3 - 2 * b13 * l1 * l3 - a13,
                        l2 * l2 + l3 * l3 - 2 * b23 * l2 * l3 - a23], axis=2)
        rel = np.abs(res).max(axis=2) / np.maximum(np.maximum(a12, a13), a23)
        assert info["alive"].any(axis=1).all()
        worst = max(worst, float(rel[info["alive"]].max()))
    print("worst relative distance residual %.2e" % worst)
    assert worst <= 1e-12


def test_every_candidate_reprojects_its_sample_onto_the_bearings(noise_free):
    """Substitution: for every candidate that survives, R X_i + t is l_i y_i for the three sample points -- a rotation, the
    points on their bearings at the polished distances."""
    worst = 0.0
    for r in noise_free:
        info = r["out"][4]
        Rc, tc = info["poses"]                                  # (H, 4, 3, 3), (H, 4, 3)
        alive = info["alive"]
        X3 = r["X"][:, :3]                                      # (H, 3, 3)
        Xc = np.einsum("hcrk,hik->hcir", Rc, X3) + tc[:, :, None, :]          # (H, 4, 3 points, 3)
        want = info["lengths"][:, :, :, None] * info["bearings"][:, None, :, :]
        scale = np.abs(want).max(axis=(2, 3))
        d = np.abs(Xc - want).max(axis=(2, 3)) / scale
        worst = max(worst, float(d[alive].max()))
        # R^T R - I is the difference of the two triangles' Gram matrices, at most the distance residuals (1e-12 max a_ij,
        # the test above), seen through the inverse Gram matrix of the world triangle, of norm about max a_ij / area2 with
        # area2 = |(X1 - X2) x (X1 - X3)|^2: a thin triangle gives a less orthogonal R. A factor 10 for the norms' constants.
        RtR = np.einsum("hcij,hcik->hcjk", Rc, Rc)
        bound = 10 * 1e-12 * (info["amax"] * info["amax"] / info["area2"])[:, None]
        assert (np.abs(RtR - np.eye(3)).max(axis=(2, 3)) <= bound)[alive].all()
        assert (np.linalg.det(Rc[alive]) > 0.999).all()
    print("worst relative distance of a sample point from its bearing %.2e" % worst)
    assert worst < 1e-9


def test_the_default_solver_is_untouched():
    """solver="dlt" results are byte-identical to calls without the keyword, in hypotheses and in estimate."""
    from aria_slam_amd import pnp_ref as N
    corr = N.synth_pnp(5, 120, *PC.motion(3), 0.3)[0]
    a = N.hypotheses(corr, 3, 5, 128)
    b = N.hypotheses(corr, 3, 5, 128, solver="dlt")
    assert all(x.tobytes() == y.tobytes() and x.dtype == y.dtype and x.shape == y.shape for x, y in zip(a, b))
    assert np.array_equal(N.sample_indices(3, 5, 128, 120), N.sample_indices(3, 5, 128, 120, k=6))
    for dtype in (None, np.longdouble):
        ea = N.estimate(corr, 3, 5, 128, dtype=dtype)
        eb = N.estimate(corr, 3, 5, 128, dtype=dtype, solver="dlt")
        assert ea.keys() == eb.keys()
        for k in ea:
            assert np.asarray(ea[k]).tobytes() == np.asarray(eb[k]).tobytes(), k
    assert N.estimate(corr[:5])["valid"] == 0 and N.estimate(corr[:5], solver="p3p")["valid"] in (0, 1)
    with pytest.raises(ValueError):
        N.estimate(corr, solver="epnp")


@pytest.mark.parametrize("case", QC.P3P_CASES + QC.P3P_BATCH, ids=QC.case_id)
def test_table_case_can_be_decided(case):
    """Conditions on the inputs, not measurements: a case that violates one is replaced, the condition stays."""
    rep = QC.report(case)
    ref, ext = rep["ref"], rep["ext"]
    assert rep["unambiguous"]                                  # no other hypothesis within the in-band points of the winner
    for k in ("valid", "best_hypothesis", "iterations", "refined", "n_inliers", "n_corr"):
        assert ext[k] == ref[k]                                # the extended run takes every decision the fp64 run takes
    assert np.array_equal(ext["mask"], ref["mask"])
    assert rep["ext_branches_equal"]                           # ... and the solver every branch, on the winner's sample
    if not ref["valid"]:
        return
    assert np.isfinite(np.asarray(ref["R"], np.float64)).all() and np.isfinite(np.asarray(ref["t"], np.float64)).all()
    assert 0 <= rep["slots"][ref["best_hypothesis"]] <= 3
    if not rep["exact"]:
        assert rep["band_winner"] == 0
        assert ref["refit_R"] is None or abs(ref["n_refit"] - ref["n_winner"]) > rep["in_band"]


def test_table_covers_the_stage():
    from aria_slam_amd import pnp_ref as N
    cases = QC.P3P_CASES
    reps = [QC.report(c) for c in cases]
    T = QC.TILE
    assert {0, 3, 4, 5, 6, 40, 150, 300, T + 1} <= {c.n for c in cases}
    assert {64, 320, 1024} <= {c.H for c in cases} and sum(c.H == 1024 for c in cases) == 1
    assert {0, 3, QC.HIGH_SEED} <= {c.seed for c in cases} and {0, 5, 1000000} <= {c.pair_base for c in cases}
    assert {0.5, 2.0, 8.0} <= {c.threshold_px for c in cases} and {QC.EUROC, QC.LOOP} <= {c.K for c in cases}
    assert {0.3, 0.5} <= {c.outliers for c in cases if c.n == 40}
    assert any(c.offset == 1000.0 and c.n == 300 for c in cases) and any(c.refine_iters == 0 for c in cases)
    assert [c.n for c in QC.P3P_BATCH] == [300, 0, 3, 4, T - 1, 5, T, 6, 40, 150]
    assert sum(not r["exact"] for r in reps) <= 2 and all(QC.report(c)["exact"] for c in QC.P3P_BATCH)
    for r in reps:
        c, ref = r["case"], r["ref"]
        if c.n < 4:
            assert ref["valid"] == 0 and r["hyp"] is None
        elif c.n < 6:                                           # valid where the DLT stage says valid = 0; no refinement
            assert ref["valid"] == 1 and ref["refined"] == 0 and ref["iterations"] == 0 and ref["n_inliers"] == c.n
            assert N.estimate(r["corr"], c.seed, c.pair_base, c.H, c.threshold_px, c.refine_iters, c.K)["valid"] == 0
        elif c.collinear or c.copies == 1.0:
            assert ref["valid"] == 0 and (r["hyp"][3] == -1).all()
        else:
            assert ref["valid"] == 1 and ref["refined"] == (1 if c.refine_iters else 0)
    # the planar cases: two motions, 0 and 30 % outliers; the DLT restatement yields valid = 0 on each
    planar = [cases[i] for i in QC.PLANAR_CASES]
    assert len({c.motion for c in planar}) == 2 and {(c.motion, c.outliers) for c in planar} == {(2, 0.0), (2, 0.3), (3, 0.0), (3, 0.3)}
    for c in planar:
        r = QC.report(c)
        assert c.n == 150 and r["ref"]["valid"] == 1 and r["ref"]["n_inliers"] > 0
        assert N.estimate(r["corr"], c.seed, c.pair_base, c.H, c.threshold_px, c.refine_iters, c.K)["valid"] == 0
    # the tie scene: every clean hypothesis counts all n, the winner is the first of them and not hypothesis 0
    tie = [r for r in reps if r["case"].noise_px == 0.0 and 0 < r["case"].copies < 1]
    assert len(tie) == 1
    counts, best = tie[0]["hyp"][3], tie[0]["ref"]["best_hypothesis"]
    assert best >= 1 and counts.max() == tie[0]["case"].n == tie[0]["ref"]["n_winner"] and (counts[:best] < counts[best]).all()
    assert (counts[best + 1:] == tie[0]["case"].n).sum() >= 1
    far = [r for r in reps if r["case"].offset == 1000.0][0]
    assert far["ref"]["n_inliers"] > 0.9 * far["case"].n * (1 - far["case"].outliers)


def test_planar_ground_truth_error_of_the_restatement():
    """The restatement's worst error over the planar cases, as tools/p3p_gap.py prints it: the numbers the GPU test doubles."""
    worst = [0.0, 0.0, 1.0]
    for i in QC.PLANAR_CASES:
        rep = QC.report(QC.P3P_CASES[i])
        r, t, prec = QC.truth_error(rep["ref"], rep)
        worst = [max(worst[0], r), max(worst[1], t), min(worst[2], prec)]
    assert abs(worst[0] - QC.PLANAR_TRUTH_ERROR[0]) < 1e-4 and abs(worst[1] - QC.PLANAR_TRUTH_ERROR[1]) < 1e-5 and worst[2] == 1.0


def test_p3p_kernel_cross_compiles_without_scratch_or_lds():
    from test_pnp_host import _listing
    text = _listing()
    body, meta = S.kernel_body(text, "k_pnp_hyp_p3p")
    assert len(body) > 200
    assert meta.get("ScratchSize", -1) == 0, meta
    in_loop, outside = S.scratch_accesses(text, "k_pnp_hyp_p3p")
    assert not in_loop and not outside
    assert meta.get("LDSByteSize", -1) == 0
    for k in ("k_pnp_hyp", "k_pnp_score"):                      # and its neighbours still have none
        assert S.kernel_body(text, k)[1].get("ScratchSize", -1) == 0, k
    src = open(os.path.join(ROOT, "aria_slam_amd", "csrc", "pnp_ransac.hip")).read()
    body_src = src[src.index("void k_pnp_hyp_p3p"):src.index("// ---- scoring")]
    for banned in ("cbrt", "acos", "cos(", "atan", "sin(", "pow("):
        assert banned not in body_src, banned
    # the hand-over has one definition, used by both hypothesis kernels
    assert len(re.findall(r"bool pnp_hand_over\(", src)) == 1 and len(re.findall(r"pnp_hand_over\(", src)) == 3
    assert len(re.findall(r"void pnp_store_model\(", src)) == 1 and len(re.findall(r"pnp_store_model\(", src)) == 3
