"""Absolute pose from the point map (include/aria_orb_hip.h, "absolute pose from the point map"): the parts that need no GPU --
exports, record layouts, the NumPy restatement (aria_slam_amd/pnp_ref.py) against ground truth and against itself, the
association rule, what the case table of tests/pnp_cases.py covers, the kernels' listing and the C++ adapter build."""
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
import pnp_cases as PC   # noqa: E402

PNP_SYMBOLS = ["aria_pnp_default_config", "aria_pnp_create", "aria_pnp_destroy", "aria_pnp_stream", "aria_pnp_check",
               "aria_pnp_estimate", "aria_pnp_estimate_batch_device", "aria_pnp_debug_hypotheses",
               "aria_pnp_associate_batch_device"]


def test_pnp_symbols_exported_and_listed(aria):
    from aria_slam_amd import _lib
    L = aria.load_library()
    header = open(os.path.join(ROOT, "include", "aria_orb_hip.h")).read()
    for name in PNP_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), "%s not declared in the header" % name
        assert hasattr(L, name), "libaria_orb_hip.so does not export %s" % name
        assert name in _lib.EXPORTS, "%s missing from _lib.EXPORTS" % name
    assert aria.abi_version() == 4
    assert aria.HipPnPEstimator.__name__ in aria.__all__


def test_pnp_record_layouts_and_defaults(aria):
    import ctypes as C
    from aria_slam_amd import _lib
    assert _lib.PNP_CORR_DTYPE.itemsize == 32              # double X[3], float u, v
    assert _lib.PNP_RESULT_DTYPE.itemsize == 128           # double R[9], t[3], rms_px + 6 ints
    assert C.sizeof(_lib.PnpConfig) == 72
    cfg = _lib.PnpConfig()
    aria.load_library().aria_pnp_default_config(C.byref(cfg))
    assert cfg.struct_size == 72 and cfg.hypotheses == 1024 and cfg.threshold_px == 2.0 and cfg.refine_iters == 5
    assert (cfg.fx, cfg.fy, cfg.cx, cfg.cy) == (458.654, 457.296, 367.215, 248.375) and cfg.seed == 0


def test_sampler_is_the_pose_stage_hash_with_six_slots():
    from aria_slam_amd import pnp_ref as N
    from aria_slam_amd import pose_ref as P
    for seed, pair, n in ((0, 0, 100), (3, 1000000, 600), (PC.HIGH_SEED, 5, 6)):
        idx = N.sample_indices(seed, pair, 64, n)
        assert idx.shape == (64, 6) and np.array_equal(idx, P.sample_indices(seed, pair, 64, n, k=6))
        assert (np.sort(idx, axis=1)[:, 1:] != np.sort(idx, axis=1)[:, :-1]).all() and idx.min() >= 0 and idx.max() < n
    assert (N.sample_indices(0, 0, 64, 5) == -1).all()      # n < 6: no sample


@pytest.mark.parametrize("k", range(4))
@pytest.mark.parametrize("offset", [0.0, 1000.0])
def test_pnp_ref_recovers_noise_free_poses(k, offset):
    """Exact correspondences: u and v are floats in the record, so each world point is moved onto the ray of its rounded
    pixel at its own depth. Every valid minimal solution is then the pose, and so is the estimate, to 1e-9 (times the
    distance of the world origin where the origin is 1000 units away)."""
    from aria_slam_amd import pnp_ref as N
    R, t = PC.motion(k)
    corr, _truth, Rt, tt = N.synth_pnp(40 + k, 100, R, t, 0.0, 0.0, offset=np.full(3, offset / np.sqrt(3.0)))
    # make the world points exact for the float pixels: keep each point's depth, move it onto the pixel's ray
    fx, fy, cx, cy = N.EUROC_K
    Xc = corr["X"] @ Rt.T + tt
    z = Xc[:, 2]
    Xc = np.stack([(corr["u"].astype(np.float64) - cx) / fx * z, (corr["v"].astype(np.float64) - cy) / fy * z, z], axis=1)
    corr["X"] = (Xc - tt) @ Rt
    st = N.stage(corr)
    idx = N.sample_indices(0, 0, 64, len(corr))
    Rh, th, ok = N.solve_minimal(st["X"][idx], st["xy"][idx])
    assert ok.sum() >= 60
    scale = max(1.0, offset)
    assert np.abs(Rh[ok] - Rt).max() < 1e-9 * scale and np.abs(th[ok] - tt).max() < 1e-9 * scale * scale
    r = N.estimate(corr, n_hyp=64)
    assert r["valid"] == 1 and r["n_inliers"] == 100 and r["mask"].all()
    assert np.abs(r["R"] - Rt).max() < 1e-9 and np.abs(r["t"] - tt).max() < 1e-9 * scale and r["rms_px"] < 1e-6
    assert abs(np.linalg.det(r["R"]) - 1.0) < 1e-12


def test_gauss_newton_jacobian_agrees_with_central_differences():
    from aria_slam_amd import pnp_ref as N
    rng = np.random.default_rng(5)
    R = N.rot([0.2, -1.0, 0.4], 33.0)
    t0 = np.array([0.3, -0.2, 6.0])
    d = rng.uniform(-2, 2, (20, 3))
    xy = rng.uniform(-0.5, 0.5, (20, 2))
    J = N.gn_jacobian(R, t0, d)
    eps = 1e-6
    for k in range(6):
        e = np.zeros(6)
        e[k] = eps
        Ep, Em = N.exp_so3(e[:3]), N.exp_so3(-e[:3])
        rp = N.residuals(Ep @ R, Ep @ t0 + e[3:], d, xy)
        rm = N.residuals(Em @ R, Em @ t0 - e[3:], d, xy)
        assert np.abs((rp - rm) / (2 * eps) - J[:, :, k]).max() < 1e-8, k
    # and a step from a perturbed pose lands on the pose the residuals vanish at
    xy0 = N.residuals(R, t0, d, np.zeros((20, 2)))
    Rp = N.exp_so3([0.01, -0.02, 0.015]) @ R
    R2, t2, steps = N.refine(Rp, t0 + [0.05, -0.03, 0.1], d, xy0, 8)
    assert steps <= 8 and np.abs(R2 - R).max() < 1e-12 and np.abs(t2 - t0).max() < 1e-11


def test_association_rule_on_a_hand_made_map():
    from aria_slam_amd import _lib
    from aria_slam_amd import pnp_ref as N
    pts = np.zeros(7, _lib.MAP_POINT_DTYPE)
    #            arena position:  0   1   2   3   4   5   6
    pts["pair"] = [4, 5, 5, 5, 5, 6, 5]
    pts["idx1"] = [2, 9, 2, 7, 2, 2, 3]
    pts["idx2"] = [1, 2, 8, 2, 0, 2, 2]
    for i in range(7):
        pts["X"][i] = (i, 10 + i, 20 + i)
    kq = np.zeros(5, _lib.KP_DTYPE)
    kq["x"] = [100, 101, 102, 103, 104]
    kq["y"] = [200, 201, 202, 203, 204]
    m = np.zeros(5, _lib.MATCH_DTYPE)
    m["query_idx"] = [4, 0, 3, 1, 2]
    m["train_idx"] = [2, 5, 7, 2, 9]
    corr, back = N.associate(pts, 5, 1, kq, m)
    # idx1 == 2 twice among pair 5 (positions 2 and 4): the lowest position; train 5 has no point; match order is kept
    assert back.tolist() == [0, 2, 3, 4]
    assert corr["X"][:, 0].tolist() == [2.0, 3.0, 2.0, 1.0]
    assert corr["u"].tolist() == [104.0, 103.0, 101.0, 102.0] and corr["v"].tolist() == [204.0, 203.0, 201.0, 202.0]
    corr2, back2 = N.associate(pts, 5, 2, kq, m)
    assert back2.tolist() == [0, 3] and corr2["X"][:, 0].tolist() == [1.0, 1.0]     # idx2 == 2 at positions 1, 3, 6
    corr3, back3 = N.associate(pts, 7, 1, kq, m)
    assert len(corr3) == 0 and len(back3) == 0


@pytest.mark.parametrize("case", PC.PNP_CASES + PC.PNP_BATCH, ids=PC.case_id)
def test_table_case_can_be_decided(case):
    """Conditions on the inputs, not measurements: a case that violates one is replaced, the condition stays."""
    rep = PC.report(case)
    ref, ext = rep["ref"], rep["ext"]
    assert rep["unambiguous"]                                  # no other hypothesis within the in-band points of the winner
    for k in ("valid", "best_hypothesis", "iterations", "refined", "n_inliers", "n_corr"):
        assert ext[k] == ref[k]                                # the extended run takes every decision the fp64 run takes
    assert np.array_equal(ext["mask"], ref["mask"])
    if not ref["valid"]:
        return
    assert np.isfinite(np.asarray(ref["R"], np.float64)).all() and np.isfinite(np.asarray(ref["t"], np.float64)).all()
    if not rep["exact"]:
        # a point of the winner's own band would change the refinement's input; and `refined` must not hang on the band
        assert rep["band_winner"] == 0
        assert ref["refit_R"] is None or abs(ref["n_refit"] - ref["n_winner"]) > rep["in_band"]


def test_table_covers_the_stage():
    reps = [PC.report(c) for c in PC.PNP_CASES]
    cases = PC.PNP_CASES
    T = PC.TILE
    assert {6, 7, 40, 150, 600, T - 1, T, T + 1, 4096} <= {c.n for c in cases}
    assert {64, 320, 1024, 4096} <= {c.H for c in cases}
    assert {0, 3, PC.HIGH_SEED} <= {c.seed for c in cases} and PC.HIGH_SEED >> 63 == 1
    assert {0, 5, 1000000} <= {c.pair_base for c in cases}
    assert {0.5, 2.0, 8.0} <= {c.threshold_px for c in cases} and {PC.EUROC, PC.LOOP} <= {c.K for c in cases}
    assert min(c.outliers for c in cases) == 0.0 and max(c.outliers for c in cases) == 0.5
    assert any(c.offset == 1000.0 for c in cases) and any(c.refine_iters == 0 for c in cases)
    assert [c.n for c in PC.PNP_BATCH] == [300, 0, T - 1, 5, T, 6, T + 1, 40, 600, 4, 150]
    # at most 3 cases have a point of the winning or the refined pose inside the band; the batch pairs have none
    assert sum(not r["exact"] for r in reps) <= 3
    assert all(PC.report(c)["exact"] for c in PC.PNP_BATCH)
    valid = [r for r in reps if r["ref"]["valid"]]
    assert all(r["ref"]["refined"] == (1 if r["case"].refine_iters else 0) for r in valid)
    for r in reps:
        c = r["case"]
        if c.copies == 1.0 or c.planar:                         # no valid hypothesis; the DLT's known limit
            assert r["ref"]["valid"] == 0 and c.n >= 6 and (r["hyp"][3] == -1).all()
    # tie scenes: every valid hypothesis counts all n, the winner is the first of them and not hypothesis 0
    ties = [r for r in valid if r["case"].noise_px == 0.0 and 0 < r["case"].copies < 1]
    assert len(ties) == 2
    for r in ties:
        counts, best = r["hyp"][3], r["ref"]["best_hypothesis"]
        assert best >= 1 and counts.max() == r["case"].n == r["ref"]["n_winner"]
        assert (counts[best + 1:] == r["case"].n).sum() >= 1 and (counts[:best] < 0).all()
    # the far-origin case is decided by the centring: scored about the origin in fp32 its winner would lose its inliers
    far = [r for r in valid if r["case"].offset == 1000.0][0]
    assert far["ref"]["n_inliers"] > 0.6 * far["case"].n * (1 - far["case"].outliers)


def test_ground_truth_set_and_its_worst_error():
    """The worst error of the restatement over PC.GT_CASES, as tools/pnp_gap.py prints it: the numbers the GPU test doubles."""
    worst = [0.0, 0.0, 1.0]
    for i in PC.GT_CASES:
        rep = PC.report(PC.PNP_CASES[i])
        r, t, prec = PC.truth_error(rep["ref"], rep)
        worst = [max(worst[0], r), max(worst[1], t), min(worst[2], prec)]
    assert len(PC.GT_CASES) >= 15
    assert abs(worst[0] - 0.6548) < 1e-3 and abs(worst[1] - 0.17379) < 1e-4 and worst[2] == 1.0


def _listing():
    csrc = os.path.join(ROOT, "aria_slam_amd", "csrc")
    out = os.path.join(ROOT, "build", "isa")
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, "pnp_ransac.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                           "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-fast-math", "-I" + os.path.join(ROOT, "include"),
                           "-I" + csrc, "--cuda-device-only", "-S", "-w", "-o", path, os.path.join(csrc, "pnp_ransac.hip")])
    return open(path).read()


def test_pnp_kernels_cross_compile_and_the_solver_and_scoring_have_no_scratch():
    text = _listing()
    for k in ("k_pnp_stage", "k_pnp_hyp", "k_pnp_score", "k_pnp_finish", "k_pnp_assoc_scatter", "k_pnp_assoc_gather"):
        body, meta = S.kernel_body(text, k)
        assert len(body) > 20, k
    for k in ("k_pnp_hyp", "k_pnp_score"):
        body, meta = S.kernel_body(text, k)
        assert meta.get("ScratchSize", -1) == 0, (k, meta)
        in_loop, outside = S.scratch_accesses(text, k)
        assert not in_loop and not outside, k
        assert meta.get("LDSByteSize", 0) <= 64 * 1024


def test_pnp_ransac_is_in_the_product_build_and_reads_no_environment():
    mk = open(os.path.join(ROOT, "aria_slam_amd", "csrc", "Makefile")).read()
    src_line = [ln for ln in mk.splitlines() if ln.startswith("SRC :=")][0]
    assert "pnp_ransac.hip" in src_line
    src = open(os.path.join(ROOT, "aria_slam_amd", "csrc", "pnp_ransac.hip")).read()
    src += "".join(open(os.path.join(ROOT, "aria_slam_amd", "csrc", h)).read() for h in ("stage_handle.h", "ransac_device.h", "solver_device.h"))
    assert "getenv" not in src
    assert "atomicAdd(float" not in src and "atomicAdd(double" not in src


def test_host_adapters_build_with_the_pnp_estimator(aria):
    pkg = os.path.join(ROOT, "aria_slam_amd")
    subprocess.check_call(["make", "-C", os.path.join(pkg, "host"), "-s"])
    so = os.path.join(pkg, "libaria_hip_adapters.so")
    syms = subprocess.run(["nm", "-DC", so], capture_output=True, text=True, check=True).stdout
    assert "aria::adapters::hip::HipPnPEstimator::estimate" in syms
    assert "aria::adapters::hip::HipPnPEstimator::estimateAgainstMap" in syms
    assert "aria::adapters::hip::MapTracker::track" in syms
    src = open(os.path.join(pkg, "host", "src", "euroc_frontend.cpp")).read()
    assert '"--track-map"' in src and "MapTracker" in src
    assert os.path.exists(os.path.join(pkg, "euroc_frontend"))


# functions elsewhere in csrc that share a name with a shared helper and are another function: other arguments, another
# summation order (merging them would change bits). Keyed by their parameter list, so a copy of the shared form still counts.
OTHER_FORMS = {
    ("block_sum", "pnp_ransac.hip", "double (&acc)[N], double (*wave)[N], double* out"),
    ("block_sum", "traj_eval.hip", "T (&v)[N], T* lds"),
    ("wave_sum", "orb_kernels.hip", "int v"),
}


def _definitions(code):
    """[(name, parameter list or None)] of the functions, constants, structs and vector typedefs a source text defines."""
    out = [(m.group(1), " ".join(m.group(2).split()))
           for m in re.finditer(r"^[ \t]*__(?:device|host)__[^\n;(]*?\b(\w+)\(([^)]*(?:\([^)]*\)[^)]*)*)\)\s*\{", code, re.M)]
    for stmt in re.findall(r"^[ \t]*constexpr\s+\w+\s+(\w+\s*=[^;(]*);", code, re.M):
        out += [(n, None) for n in re.findall(r"(\w+)\s*=", stmt)]
    out += [(n, None) for n in re.findall(r"^[ \t]*struct\s+(\w+)\s*\{", code, re.M)]
    out += [(n, None) for n in re.findall(r"^[ \t]*typedef\s[^;]*?\b(\w+)\s+__attribute__\(\(ext_vector_type", code, re.M)]
    return out


def test_shared_device_helpers_have_one_definition():
    """Every helper of solver_device.h and of graph_lm_device.h, and the packed-int16 helpers of orb_device.h, is defined once
    among csrc/*.hip and csrc/*.h, in its shared header, and every .hip that uses it includes that header: no second copy to
    drift from the first."""
    csrc = os.path.join(ROOT, "aria_slam_amd", "csrc")
    strip = lambda t: re.sub(r"//[^\n]*", "", t)   # noqa: E731
    code = {f: strip(open(os.path.join(csrc, f)).read()) for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h"))}
    # the names at file scope of solver_device.h (LmDamping's members are indented and belong to it)
    unindented = "\n".join(ln for ln in code["solver_device.h"].splitlines() if not ln.startswith((" ", "\t")))
    solver = sorted({n for n, _ in _definitions(unindented)})
    assert set(solver) >= {"jacobi_rotate", "jacobi3", "wave_sum", "block_sum2", "block_sum", "block_max", "tri6", "exp_so3",
                           "LmDamping", "LM_MAX_TRIALS", "STOP_ITERATIONS", "STOP_TRIALS", "STOP_INVALID"}, solver
    shared = [(n, "solver_device.h") for n in solver]
    shared += [(n, "orb_device.h") for n in ("short2v", "pk_min_i16", "pk_max_i16", "pk_sub_i16", "pk_add_i16")]
    # the same for graph_lm_device.h: the pieces k_graph_lm and k_sgraph_lm share (GraphScratch's members belong to it), and
    # the host templates around the kernels, which carry no __host__ for _definitions to see
    # (its signatures run over two lines, so the indented lines stay and the indented definitions are masked)
    file_scope = re.sub(r"(?m)^[ \t]+(?=__device__|__host__|struct\b|constexpr\b|typedef\b)", "    masked ", code["graph_lm_device.h"])
    graph_lm = sorted({n for n, _ in _definitions(file_scope)})
    assert set(graph_lm) >= {"GraphScratch", "LmRed", "lm_stride", "sym_idx", "unit_quat_from_rot", "rot_from_quat", "load_pose",
                             "mul_tn", "mul_nn", "mulv_t", "rotation_update", "edge_pass", "build_adjacency", "vertex_gather",
                             "precond_build", "precond_apply", "pcg_solve"}, graph_lm
    shared += [(n, "graph_lm_device.h") for n in graph_lm]
    host = {f: re.findall(r"^(?:int|void)\s+(graph_lm_\w+)\(", text, re.M) for f, text in code.items()}
    assert sorted(host.pop("graph_lm_device.h")) == ["graph_lm_debug_linearize", "graph_lm_launch", "graph_lm_optimize",
                                                     "graph_lm_optimize_batch_device", "graph_lm_reserve",
                                                     "graph_lm_stage_single"] and not any(host.values()), host
    for f in ("graph_optimize.hip", "sim3_graph.hip"):            # both stages go through every one of them
        for n in ("graph_lm_reserve", "graph_lm_optimize", "graph_lm_optimize_batch_device", "graph_lm_debug_linearize"):
            assert n + "<" in code[f], (f, n)
    for name, header in shared:
        where = [f for f, text in code.items() for n, params in _definitions(text)
                 if n == name and (name, f, params) not in OTHER_FORMS]
        assert where == [header], (name, where)
        own = {f for n, f, _ in OTHER_FORMS if n == name}        # these may use their own function of that name
        for f, text in code.items():
            if f.endswith(".hip") and f not in own and re.search(r"\b%s\b" % name, text):
                assert '#include "%s"' % header in text, (name, f)
    found = {(n, f, p) for f, text in code.items() for n, p in _definitions(text)}
    assert OTHER_FORMS <= found, OTHER_FORMS - found            # no stale exception
