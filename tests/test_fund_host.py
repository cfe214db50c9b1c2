"""Fundamental-matrix RANSAC (include/aria_orb_hip.h, "fundamental-matrix RANSAC"): the parts that need no GPU -- exports and
layouts, the NumPy restatement (aria_slam_amd/fund_ref.py) against ground truth and against an SVD basis, the sample hash at
k = 7, the kernels' listing and the C++ adapter build."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_kernel_stats as S   # noqa: E402

FUND_SYMBOLS = ["aria_fund_default_config", "aria_fund_create", "aria_fund_destroy", "aria_fund_stream", "aria_fund_check",
                "aria_fund_estimate", "aria_fund_estimate_batch_device", "aria_fund_debug_hypotheses"]


def test_fund_symbols_exported_and_listed(aria):
    from aria_slam_amd import _lib
    L = aria.load_library()
    header = open(os.path.join(ROOT, "include", "aria_orb_hip.h")).read()
    for name in FUND_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), "%s not declared in the header" % name
        assert hasattr(L, name), "libaria_orb_hip.so does not export %s" % name
        assert name in _lib.EXPORTS, "%s missing from _lib.EXPORTS" % name
    assert aria.abi_version() == 4
    assert aria.HipFundamentalEstimator and aria.verify_loop_candidates


def test_fund_record_layouts_and_defaults(aria):
    from aria_slam_amd import _lib
    assert _lib.FUND_RESULT_DTYPE.itemsize == 96                # double F[9] + 6 ints
    assert C.sizeof(_lib.FundConfig) == 40
    cfg = _lib.FundConfig()
    aria.load_library().aria_fund_default_config(C.byref(cfg))
    assert cfg.struct_size == 40 and cfg.hypotheses == 1024 and cfg.threshold_px == 3.0 and cfg.seed == 0


def _splitmix64(x):
    m = (1 << 64) - 1
    x = (x + 0x9E3779B97F4A7C15) & m
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & m
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & m
    return x ^ (x >> 31)


def _samples_int(seed, pair, h, n, k):
    """The header's definition in plain Python integers, k slots."""
    key = _splitmix64(_splitmix64(_splitmix64(seed) ^ pair) ^ h)
    out = []
    for j in range(k):
        for retry in range(256):
            v = ((_splitmix64(key ^ (8 * retry + j)) >> 32) * n) >> 32
            if v not in out:
                out.append(v)
                break
    return out


KNOWN7 = [((0, 0, 100), [[12, 16, 31, 41, 22, 92, 46], [85, 13, 10, 61, 71, 49, 50], [89, 83, 36, 47, 95, 31, 5]]),
          ((1, 7, 600), [[26, 524, 195, 103, 263, 434, 594], [591, 116, 122, 589, 194, 234, 343],
                         [147, 481, 569, 574, 319, 571, 282]]),
          ((12345, 4095, 15), [[1, 7, 4, 2, 13, 3, 14], [8, 7, 5, 6, 2, 1, 14], [12, 6, 0, 7, 13, 8, 2]])]


@pytest.mark.parametrize("args,want", KNOWN7)
def test_sample_hash_known_answers_k7(args, want):
    from aria_slam_amd import fund_ref as F, pose_ref as P
    seed, pair, n = args
    assert [_samples_int(seed, pair, h, n, 7) for h in range(3)] == want
    assert P.sample_indices(seed, pair, 3, n, k=7).tolist() == want
    assert F.sample_indices(seed, pair, 3, n).tolist() == want
    assert P.sample_indices(seed, pair, 3, n).tolist() == [_samples_int(seed, pair, h, n, 8) for h in range(3)]   # k = 8 unchanged
    assert (F.sample_indices(seed, pair, 64, 14) == -1).all()          # n < 15: no sample


def _motion():
    from aria_slam_amd import pose_ref as P
    R, t = P.rot([0.1, 1.0, 0.2], 10.0), np.array([0.6, 0.1, 0.8])
    return R, t / np.linalg.norm(t)


def _scene(seed=3, n=100, noise=0.0, outliers=0.0):
    from aria_slam_amd import fund_ref as F
    R, t = _motion()
    kq, kt, m, truth = F.synth_two_view(seed, n, R, t, outliers, noise_px=noise)
    return kq, kt, m, truth, F.true_fundamental(R, t)


def _exact_pixels(n, seed):
    """(n, 4) fp64 pixel pairs of the scene, exact (not rounded to fp32): K = 700 / 700 / 320 / 180 at 640x360."""
    from aria_slam_amd import fund_ref as F
    fx, fy, cx, cy = F.REFERENCE_LOOP_K
    R, t = _motion()
    rng = np.random.default_rng(seed)
    u, v, z = rng.uniform(0, 640, n), rng.uniform(0, 360, n), rng.uniform(2, 20, n)
    Y = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1) @ R.T + t
    return np.stack([u, v, fx * Y[:, 0] / Y[:, 2] + cx, fy * Y[:, 1] / Y[:, 2] + cy], 1)


def test_seven_point_recovers_the_true_f_and_satisfies_its_sample():
    from aria_slam_amd import fund_ref as F
    R, t = _motion()
    Ft = F.true_fundamental(R, t)
    samples = _exact_pixels(300, 1)[:70].reshape(10, 7, 4)
    Fm, nm = F.solve7(samples)
    assert (nm >= 1).all()
    for h in range(len(samples)):
        err = min(np.abs(Fm[h, k] - Ft.ravel()).max() / np.abs(Ft).max() for k in range(nm[h]))
        assert err < 1e-8, (h, err)
        x1 = np.c_[samples[h, :, :2], np.ones(7)]
        x2 = np.c_[samples[h, :, 2:], np.ones(7)]
        for k in range(nm[h]):
            M = Fm[h, k].reshape(3, 3)
            assert abs(np.linalg.det(M)) < 1e-9 * np.linalg.norm(M) ** 3
            r = np.einsum("ij,jk,ik->i", x2, M, x1)
            assert np.abs(r).max() < 1e-9 * np.linalg.norm(M) * 640 * 640, r
            assert abs(M[2, 2] - 1.0) < 1e-15


def test_seven_point_models_do_not_depend_on_the_basis():
    """run7Point takes its basis from the SVD; the stage from elimination. The rank-2 pencil members are the same: to 1e-9
    of the model's largest entry for all but the few near-degenerate samples, whose conditioning amplifies rounding."""
    from aria_slam_amd import fund_ref as F
    kq, kt, m, _, _ = _scene(5, 300, 0.5, 0.3)
    pts = F.pixels(kq, kt, m)
    idx = F.sample_indices(0, 0, 256, len(pts))
    Fa, na = F.solve7(pts[idx])
    Fb, nb = F.solve7(pts[idx], basis="svd")
    assert (na == nb).mean() > 0.99 and (na > 0).mean() > 0.95
    dev = []
    for h in np.flatnonzero((na == nb) & (na > 0)):
        A, B = Fa[h, :na[h]], Fb[h, :nb[h]]
        scale = np.abs(A).max()
        # the SVD form's roots come in another order: match model to model
        dev.append(max(np.abs(B - a).max(axis=1).min() / scale for a in A))
    dev = np.array(dev)
    assert (dev <= 1e-9).mean() >= 0.98 and dev.max() < 1e-4, np.percentile(dev, [50, 99, 100])


@pytest.mark.parametrize("seed", range(6))
def test_cubic_matches_numpy_roots(seed):
    from aria_slam_amd import fund_ref as F
    rng = np.random.default_rng(seed)
    for want_three in (True, False):
        for _ in range(50):
            r = rng.uniform(-5, 5, 3) if want_three else np.array([rng.uniform(-5, 5), 0, 0])
            if want_three:
                c = np.poly(r) * rng.uniform(0.5, 3)
            else:
                re_, im = rng.uniform(-5, 5), rng.uniform(0.5, 3)
                c = np.poly([r[0], re_ + 1j * im, re_ - 1j * im]).real * rng.uniform(0.5, 3)
            got, n = F.cubic_roots(c[None])
            want = np.sort(np.roots(c).real[np.abs(np.roots(c).imag) < 1e-9])
            assert n[0] == (3 if want_three else 1)
            assert np.allclose(got[0, :n[0]], want, rtol=1e-7, atol=1e-7), (got, want)
    got, n = F.cubic_roots(np.array([[1e-14, 1.0, 2.0, 3.0]]))
    assert n[0] == 0                                                  # |c0| <= 1e-12 max|c_i|: no cubic


def test_error_function_hand_computed():
    from aria_slam_amd import fund_ref as F
    # F = [e]x with e = (1, 0, 0): epipolar lines of view 2 are horizontal, x2^T F x1 = y1 - y2 (up to sign)
    Fm = np.array([0, 0, 0, 0, 0, -1, 0, 1, 0], np.float64)
    pts = np.array([[10, 20, 30, 23], [5, 5, 7, 5], [0, 0, 0, 10]], np.float32)
    e = F.errors(Fm, pts)[0]
    # a = F x1 = (0, -1, y1): distance of x2 = |y2 - y1|; symmetric; max = (y2 - y1)^2
    assert e.tolist() == [9.0, 0.0, 100.0]
    assert (e <= F.threshold2(3.0)).tolist() == [True, True, False]
    assert np.isinf(F.errors(np.zeros(9), pts)).all()                   # zero line normal: never an inlier


def test_degenerate_samples_are_invalid():
    from aria_slam_amd import fund_ref as F
    rng = np.random.default_rng(1)
    good = rng.uniform(0, 600, (7, 4)).astype(np.float32)
    col = good.copy()
    col[6, 0] = 0.5 * (col[0, 0] + col[1, 0])                          # slot 6 on the line through slots 0 and 1 (view 1)
    col[6, 1] = 0.5 * (col[0, 1] + col[1, 1])
    col[0, :2], col[1, :2] = [100.0, 100.0], [300.0, 200.0]
    col[6, :2] = [200.0, 150.0]
    assert F.collinear(col[None, :, 0], col[None, :, 1])[0]
    same = good.copy()
    same[:, 2:] = same[:, :2]                                          # x1 == x2 for every match: rank 6
    Fm, nm = F.solve7(np.stack([good, col, same]))
    assert nm.tolist()[1:] == [0, 0] and nm[0] in (1, 3)
    assert not Fm[1:].any() and np.isfinite(Fm).all()


@pytest.mark.parametrize("outliers", [0.0, 0.2, 0.4])
def test_fund_ref_ransac_ground_truth(outliers):
    from aria_slam_amd import fund_ref as F
    for seed in (11, 12):
        kq, kt, m, truth, _ = _scene(seed, 200, 0.5, outliers)
        r = F.estimate(kq, kt, m)
        assert r["valid"] == 1 and r["n_inliers"] == int(r["mask"].sum()) and r["n_models"] > 1024
        e = np.sqrt(F.errors(r["F"].ravel(), F.pixels(kq, kt, m))[0].astype(np.float64))
        assert np.median(e[truth]) < 1.0
        sel = r["mask"] == 1
        assert truth[sel].mean() >= 0.95


def test_fund_ref_edges():
    from aria_slam_amd import fund_ref as F
    kq, kt, m, _, _ = _scene(5, 40, 0.5)
    for n in (0, 7, 14):
        r = F.estimate(kq, kt, m[:n])
        assert r["valid"] == 0 and not r["mask"].any() and not r["F"].any() and r["best_hypothesis"] == -1
    assert F.estimate(kq, kt, m[:15])["valid"] == 1
    same = m.copy()
    same["train_idx"] = same["query_idx"]
    r = F.estimate(kq, kq, same)                                       # identical points in both views
    assert r["valid"] == 0 and np.isfinite(r["F"]).all()


def _listing():
    csrc = os.path.join(ROOT, "aria_slam_amd", "csrc")
    out = os.path.join(ROOT, "build", "isa")
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, "fund_ransac.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                           "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-fast-math", "-I" + os.path.join(ROOT, "include"),
                           "-I" + csrc, "--cuda-device-only", "-S", "-w", "-o", path, os.path.join(csrc, "fund_ransac.hip")])
    return open(path).read()


def test_fund_kernels_cross_compile_and_scoring_has_no_scratch():
    text = _listing()
    for k in ("k_fund_stage", "k_fund_hyp", "k_fund_score", "k_fund_finish"):
        body, meta = S.kernel_body(text, k)
        assert len(body) > 50, k
    body, meta = S.kernel_body(text, "k_fund_score")
    assert meta.get("ScratchSize", -1) == 0, meta
    in_loop, outside = S.scratch_accesses(text, "k_fund_score")
    assert not in_loop and not outside
    assert meta.get("LDSByteSize", 0) <= 64 * 1024


def test_fund_ransac_is_in_the_product_build_and_reads_no_environment():
    mk = open(os.path.join(ROOT, "aria_slam_amd", "csrc", "Makefile")).read()
    src_line = [ln for ln in mk.splitlines() if ln.startswith("SRC :=")][0]
    assert "fund_ransac.hip" in src_line
    src = open(os.path.join(ROOT, "aria_slam_amd", "csrc", "fund_ransac.hip")).read()
    # the rules below follow the code into the shared headers this file includes
    src += "".join(open(os.path.join(ROOT, "aria_slam_amd", "csrc", h)).read() for h in ("stage_handle.h", "ransac_device.h") if '#include "%s"' % h in src)
    assert "getenv" not in src and "atomicAdd(&" not in src.replace("atomicAdd(&n_models", "")


def test_host_adapters_build_with_the_reference_verifier(aria):
    pkg = os.path.join(ROOT, "aria_slam_amd")
    subprocess.check_call(["make", "-C", os.path.join(pkg, "host"), "-s"])
    syms = subprocess.run(["nm", "-DC", os.path.join(pkg, "libaria_hip_adapters.so")], capture_output=True, text=True,
                          check=True).stdout
    assert "aria::adapters::hip::makeReferenceVerifier" in syms
    usage = subprocess.run([os.path.join(pkg, "euroc_frontend")], capture_output=True, text=True)
    assert "--loop-verify" in usage.stderr


# ---- the case table of the GPU tests (tests/ransac_cases.py): what it covers, proven with the restatement alone ------------
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ransac_cases as RC   # noqa: E402


@pytest.mark.parametrize("case", RC.FUND_CASES + RC.FUND_BATCH, ids=RC.case_id)
def test_table_case_can_be_decided(case):
    """Conditions on the inputs, not measurements: a case that violates one is replaced, the condition stays."""
    from aria_slam_amd import fund_ref as F
    rep = RC.fund_report(case)
    assert rep["unambiguous"]                                   # no other model within the in-band points of the winner
    assert rep["in_band"] <= RC.in_band_limit(case.n)
    if rep["ref"]["valid"]:
        assert rep["F_ext"] is not None                         # the extended solve finds the same number of roots
        assert rep["ref"]["n_inliers"] >= F.MIN_INLIERS


def test_table_covers_the_finish_kernel():
    from aria_slam_amd import fund_ref as F
    cases = RC.FUND_CASES
    reps = [RC.fund_report(c) for c in cases]
    assert {15, 16, 40, 150, 300, 600, 2047, 2048, 2049, 4096} <= {c.n for c in cases}
    assert {64, 320, 1024, 4096} <= {c.H for c in cases}
    assert {0, 3, RC.HIGH_SEED} <= {c.seed for c in cases} and {0, 5, 1000000} <= {c.pair_base for c in cases}
    assert {1.0, 3.0} <= {c.threshold_px for c in cases} and {True, False} <= {c.query_is_first for c in cases}
    valid = [r for r in reps if r["ref"]["valid"]]
    assert {r["ref"]["best_root"] for r in valid} == {0, 1, 2}
    assert any(not r["ref"]["valid"] and r["case"].n >= F.MIN_MATCHES for r in reps)     # fails MIN_INLIERS
    assert sum(r["exact"] for r in reps) >= 0.8 * len(reps) and not all(r["exact"] for r in reps)
    # tie scenes: the true F takes all n wherever it is among a sample's roots; the winner is the lowest (h, root) of them
    ties = [r for r in valid if r["case"].noise_px == 0.0 and 0 < r["case"].copies < 1]
    winners = sorted(r["ref"]["best_hypothesis"] for r in ties)
    assert winners[0] >= 1 and winners[-1] >= 256
    for r in ties:
        c = r["case"]
        _idx, _nm, _F, counts = F.hypotheses(r["pts"], c.seed, c.pair_base, c.H, c.threshold_px)
        flat = counts.reshape(-1)
        best = 3 * r["ref"]["best_hypothesis"] + r["ref"]["best_root"]
        assert flat.max() == c.n == r["ref"]["n_inliers"]
        assert (flat[best + 1:] == c.n).sum() >= 1 and (flat[:best] < c.n).all()


def test_solve7_extended_run_follows_the_fp64_run():
    """The np.longdouble run of solve7 (the yardstick of the device's F) takes the fp64 run's decisions and lands on its
    models wherever the sample is well conditioned."""
    from aria_slam_amd import fund_ref as F
    rep = RC.fund_report(RC.FUND_CASES[8])
    c = rep["case"]
    idx = F.sample_indices(c.seed, c.pair_base, 256, c.n)
    a, na = F.solve7(rep["pts"][idx])
    b, nb = F.solve7(rep["pts"][idx], dtype=np.longdouble)
    assert b.dtype == np.longdouble and (na == nb).mean() > 0.99
    same = na == nb
    sc = np.abs(b[same]).max(axis=2, keepdims=True)
    sc[sc == 0] = 1
    d = np.abs(a[same] / sc - b[same] / sc).max(axis=(1, 2)).astype(np.float64)
    assert np.median(d) < 1e-14
