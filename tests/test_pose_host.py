"""Two-view relative pose (include/aria_orb_hip.h, "two-view relative pose"): the parts that need no GPU -- exports, the NumPy
restatement (aria_slam_amd/pose_ref.py) against ground truth, the sample hash, the kernels' listing and the C++ adapter build."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_kernel_stats as S   # noqa: E402

POSE_SYMBOLS = ["aria_pose_default_config", "aria_pose_create", "aria_pose_destroy", "aria_pose_stream", "aria_pose_check",
                "aria_pose_estimate", "aria_pose_estimate_batch_device", "aria_pose_debug_hypotheses"]


def test_pose_symbols_exported_and_listed(aria):
    from aria_slam_amd import _lib
    L = aria.load_library()
    header = open(os.path.join(ROOT, "include", "aria_orb_hip.h")).read()
    for name in POSE_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), "%s not declared in the header" % name
        assert hasattr(L, name), "libaria_orb_hip.so does not export %s" % name
        assert name in _lib.EXPORTS, "%s missing from _lib.EXPORTS" % name
    assert aria.abi_version() == 4


def test_pose_record_layouts(aria):
    import ctypes as C
    from aria_slam_amd import _lib
    assert _lib.POSE_RESULT_DTYPE.itemsize == 192          # double R[9], t[3], E[9] + 6 ints
    assert C.sizeof(_lib.PoseConfig) == 80
    cfg = _lib.PoseConfig()
    aria.load_library().aria_pose_default_config(C.byref(cfg))
    assert cfg.struct_size == 80 and cfg.hypotheses == 1024 and cfg.threshold_px == 1.0 and cfg.distance_thresh == 50.0
    assert (cfg.fx, cfg.fy, cfg.cx, cfg.cy) == (458.654, 457.296, 367.215, 248.375)


def _splitmix64(x):
    m = (1 << 64) - 1
    x = (x + 0x9E3779B97F4A7C15) & m
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & m
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & m
    return x ^ (x >> 31)


def _samples_int(seed, pair, h, n):
    """The header's definition in plain Python integers."""
    key = _splitmix64(_splitmix64(_splitmix64(seed) ^ pair) ^ h)
    out = []
    for j in range(8):
        for retry in range(256):
            v = ((_splitmix64(key ^ (8 * retry + j)) >> 32) * n) >> 32
            if v not in out:
                out.append(v)
                break
    return out


KNOWN = [((0, 0, 100), [[12, 16, 31, 41, 22, 92, 46, 82], [85, 13, 10, 61, 71, 49, 50, 97], [89, 83, 36, 47, 95, 31, 5, 82]]),
         ((1, 7, 600), [[26, 524, 195, 103, 263, 434, 594, 589], [591, 116, 122, 589, 194, 234, 343, 16],
                        [147, 481, 569, 574, 319, 571, 282, 437]]),
         ((12345, 4095, 8), [[0, 3, 2, 1, 7, 4, 5, 6], [4, 5, 2, 3, 1, 0, 7, 6], [6, 3, 0, 2, 7, 4, 1, 5]])]


@pytest.mark.parametrize("args,want", KNOWN)
def test_sample_hash_known_answers(args, want):
    from aria_slam_amd import pose_ref as P
    seed, pair, n = args
    assert [_samples_int(seed, pair, h, n) for h in range(3)] == want
    assert P.sample_indices(seed, pair, 3, n).tolist() == want
    assert (P.sample_indices(seed, pair, 64, 7) == -1).all()          # n < 8: no sample


MOTIONS = {
    "forward": (np.eye(3), [0.0, 0.0, 1.0]),
    "sideways": (np.eye(3), [1.0, 0.0, 0.0]),
    "diagonal_rot5": ("rot5", [1.0, 0.3, 1.0]),
    "yaw15": ("yaw15", [0.5, 0.0, 1.0]),
}


def motion(name):
    from aria_slam_amd import pose_ref as P
    R, t = MOTIONS[name]
    if isinstance(R, str):
        R = P.rot([0.3, 1.0, 0.2], 5.0) if R == "rot5" else P.rot([0.0, 1.0, 0.0], 15.0)
    t = np.asarray(t, np.float64)
    return R, t / np.linalg.norm(t)


@pytest.mark.parametrize("name", sorted(MOTIONS))
@pytest.mark.parametrize("outliers", [0.0, 0.2])
def test_pose_ref_recovers_ground_truth(name, outliers):
    """Points at 2-20 m, sigma = 0.5 px, unit baseline (so every point lies within recoverPose's distance bound of 50)."""
    from aria_slam_amd import pose_ref as P
    R, t = motion(name)
    kq, kt, m, truth = P.synth_two_view(11, 200, R, t, outliers)
    r = P.estimate(kq, kt, m)
    assert r["valid"] == 1
    assert P.rotation_error_deg(r["R"], R) < 0.5
    assert P.angle_deg(r["t"], t) < 3.0
    sel = r["mask"] == 1
    assert truth[sel].mean() >= 0.95 and sel[truth].mean() >= 0.8, (truth[sel].mean(), sel[truth].mean())
    assert abs(np.linalg.norm(r["t"]) - 1.0) < 1e-9 and abs(np.linalg.det(r["R"]) - 1.0) < 1e-9
    assert r["n_pose_inliers"] == int(r["mask"].sum()) <= r["n_inliers"]


def test_pose_ref_minimal_solver_satisfies_its_sample():
    from aria_slam_amd import pose_ref as P
    R, t = motion("yaw15")
    kq, kt, m, _ = P.synth_two_view(3, 100, R, t, 0.0, noise_px=0.0)
    pts = P.normalise(kq, kt, m)
    idx, E, counts = P.hypotheses(pts, n_hyp=64)
    ok = counts >= 0
    assert ok.sum() >= 60            # a near-degenerate sample may fall under the pivot tolerance
    # noise-free points: every minimal solution is the true E (up to sign) and takes every point
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Eg = (tx @ R).ravel()
    Eg /= np.linalg.norm(Eg)
    assert np.allclose(np.abs(E[ok] @ Eg), 1.0, atol=1e-6)
    assert (counts[ok] == 100).all()


def test_pose_ref_edges():
    from aria_slam_amd import pose_ref as P
    R, t = motion("forward")
    kq, kt, m, _ = P.synth_two_view(5, 20, R, t)
    for n in (0, 7):
        r = P.estimate(kq, kt, m[:n])
        assert r["valid"] == 0 and not r["mask"].any() and np.array_equal(r["R"], np.eye(3)) and not r["t"].any()
    one = m.copy()
    one["query_idx"] = 0
    one["train_idx"] = 0
    r = P.estimate(kq, kt, one)
    assert r["valid"] == 0 and np.isfinite(r["R"]).all() and np.isfinite(r["t"]).all()


def _listing():
    csrc = os.path.join(ROOT, "aria_slam_amd", "csrc")
    out = os.path.join(ROOT, "build", "isa")
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, "pose_ransac.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                           "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-fast-math", "-I" + os.path.join(ROOT, "include"),
                           "-I" + csrc, "--cuda-device-only", "-S", "-w", "-o", path, os.path.join(csrc, "pose_ransac.hip")])
    return open(path).read()


def test_pose_kernels_cross_compile_and_scoring_has_no_scratch():
    text = _listing()
    for k in ("k_pose_stage", "k_pose_hyp", "k_pose_score", "k_pose_finish"):
        body, meta = S.kernel_body(text, k)
        assert len(body) > 50, k
    body, meta = S.kernel_body(text, "k_pose_score")
    assert meta.get("ScratchSize", -1) == 0, meta
    in_loop, outside = S.scratch_accesses(text, "k_pose_score")
    assert not in_loop and not outside
    assert meta.get("LDSByteSize", 0) <= 64 * 1024


def test_pose_ransac_is_in_the_product_build_and_reads_no_environment():
    mk = open(os.path.join(ROOT, "aria_slam_amd", "csrc", "Makefile")).read()
    src_line = [ln for ln in mk.splitlines() if ln.startswith("SRC :=")][0]
    assert "pose_ransac.hip" in src_line
    src = open(os.path.join(ROOT, "aria_slam_amd", "csrc", "pose_ransac.hip")).read()
    # the rules below follow the code into the shared headers this file includes
    src += "".join(open(os.path.join(ROOT, "aria_slam_amd", "csrc", h)).read() for h in ("stage_handle.h", "ransac_device.h", "solver_device.h") if '#include "%s"' % h in src)
    assert "getenv" not in src


def test_host_adapters_build_with_the_pose_estimator(aria):
    pkg = os.path.join(ROOT, "aria_slam_amd")
    subprocess.check_call(["make", "-C", os.path.join(pkg, "host"), "-s"])
    so = os.path.join(pkg, "libaria_hip_adapters.so")
    syms = subprocess.run(["nm", "-DC", so], capture_output=True, text=True, check=True).stdout
    assert "aria::adapters::hip::HipPoseEstimator::estimate" in syms
    assert "aria::adapters::hip::makeGeometricVerifier" in syms
    assert os.path.exists(os.path.join(pkg, "euroc_frontend"))


# ---- the case table of the GPU tests (tests/ransac_cases.py): what it covers, proven with the restatement alone ------------
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ransac_cases as RC   # noqa: E402


@pytest.mark.parametrize("case", RC.POSE_CASES + RC.POSE_BATCH, ids=RC.case_id)
def test_table_case_can_be_decided(case):
    """Conditions on the inputs, not measurements: a case that violates one is replaced, the condition stays."""
    rep = RC.pose_report(case)
    ref = rep["ref"]
    assert rep["unambiguous"]                                   # no other hypothesis within the in-band points of the winner
    assert rep["in_band"] <= RC.in_band_limit(case.n)
    for k in ("valid", "best_hypothesis", "refined", "n_inliers", "n_pose_inliers"):
        assert rep["ext"][k] == ref[k]                          # the extended run takes every decision the fp64 run takes
    assert np.array_equal(rep["ext"]["mask"], ref["mask"])
    if not ref["valid"]:
        return
    assert rep["margin"] > rep["near"]                          # the chosen candidate beats the other three outright
    if not rep["exact"]:
        # a point of the winner's own band would change the refit's input, and with it decisions outside any band; and
        # `refined` must not hang on the in-band points
        assert rep["band_winner"] == 0
        assert ref["refit_E"] is None or abs(ref["n_refit"] - ref["n_winner"]) > rep["in_band"]


def test_table_covers_the_finish_kernel():
    reps = [RC.pose_report(c) for c in RC.POSE_CASES]
    cases = RC.POSE_CASES
    assert {8, 9, 40, 150, 300, 600, 2047, 2048, 2049, 4096} <= {c.n for c in cases}
    assert {64, 320, 1024, 4096} <= {c.H for c in cases}
    assert {0, 3, RC.HIGH_SEED} <= {c.seed for c in cases} and RC.HIGH_SEED >> 63 == 1
    assert {0, 5, 1000000} <= {c.pair_base for c in cases}
    assert {0.25, 1.0, 3.0} <= {c.threshold_px for c in cases} and {50.0, 5.0} <= {c.distance_thresh for c in cases}
    assert {RC.EUROC, RC.LOOP} <= {c.K for c in cases} and {True, False} <= {c.query_is_first for c in cases}
    valid = [r for r in reps if r["ref"]["valid"]]
    assert {r["ref"]["refined"] for r in valid} == {0, 1}
    assert any(r["ref"]["n_winner"] < 8 for r in valid)                       # no refit runs
    assert {r["ref"]["candidate"] for r in valid} == {0, 1, 2, 3}
    assert any(not r["ref"]["valid"] and r["case"].n >= 8 for r in reps)      # no valid hypothesis
    # with distance_thresh = 5 part of the inliers of a 2-20 m scene fails the depth test
    assert any(r["case"].distance_thresh == 5.0 and 0 < r["ref"]["n_pose_inliers"] < r["ref"]["n_inliers"] for r in valid)
    assert sum(r["exact"] for r in reps) >= 0.8 * len(reps) and not all(r["exact"] for r in reps)
    # tie scenes: every valid hypothesis counts all n, the winner is the first of them -- one beyond hypothesis 0 and one
    # beyond the first stride of the finish block, each with a later hypothesis at the same count
    ties = [r for r in valid if r["case"].noise_px == 0.0 and 0 < r["case"].copies < 1]
    winners = sorted(r["ref"]["best_hypothesis"] for r in ties)
    assert winners[0] >= 1 and winners[-1] >= 256
    for r in ties:
        c = r["case"]
        _idx, _E, counts = _case_hypotheses(r)
        assert counts.max() == c.n == r["ref"]["n_winner"]
        assert (counts[r["ref"]["best_hypothesis"] + 1:] == c.n).sum() >= 1 and (counts[:r["ref"]["best_hypothesis"]] < c.n).all()


def _case_hypotheses(rep):
    from aria_slam_amd import pose_ref as P
    c = rep["case"]
    return P.hypotheses(rep["pts"], c.seed, c.pair_base, c.H, c.threshold_px, c.K)


def test_extended_path_agrees_with_lapack():
    """jacobi_eigh in np.longdouble against LAPACK in fp64 on a refit's normal matrix, and the Jacobi decomposition against
    the SVD one as sets of four candidates."""
    from aria_slam_amd import pose_ref as P
    rep = RC.pose_report(RC.POSE_CASES[9])
    pts = rep["pts"]
    A = P.design_rows(pts[rep["ref"]["mask"] == 1])
    w, V = np.linalg.eigh(A.T @ A)
    wx, Vx = P.jacobi_eigh((A.astype(np.longdouble)).T @ A.astype(np.longdouble))
    assert wx.dtype == np.longdouble and np.abs(w - wx.astype(np.float64)).max() <= 1e-12 * w.max()
    assert abs(abs(float(V[:, 0] @ Vx[:, 0].astype(np.float64))) - 1.0) < 1e-12
    assert np.abs((Vx.T @ Vx).astype(np.float64) - np.eye(9)).max() < 1e-17
    a = P.decompose_essential(rep["ref"]["E"])
    b = P.decompose_essential(rep["ref"]["E"], np.longdouble)
    for R, t in a:
        assert min(max(np.abs(R - R2.astype(np.float64)).max(), np.abs(t - t2.astype(np.float64)).max()) for R2, t2 in b) < 1e-13
