"""The absolute pose stage with the P3P minimal solver on the MI355X (aria_pnp_set_solver; k_pnp_hyp_p3p in
aria_slam_amd/csrc/pnp_ransac.hip): the whole stage against pnp_ref.estimate(solver="p3p") over the case table of
tests/p3p_cases.py, hypotheses against the restatement, the planar scenes the solver exists for, switching solvers on one
handle, batch == single and determinism, edge cases, the device chain, the C++ adapters and the driver flag.
aria_slam_amd/pnp_ref.py is the definition; parity with OpenCV's SOLVEPNP_P3P is not claimed."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import p3p_cases as QC   # noqa: E402
import pnp_cases as PC   # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "aria_slam_amd")
REC = 128                                                    # bytes of an aria_pnp_result
CORR = 32                                                    # bytes of an aria_pnp_corr
E_INVALID = -1


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def est(aria):
    e = aria.HipPnPEstimator(solver="p3p")
    yield e
    e.close()


def _estimator(aria, c, solver="p3p"):
    return aria.HipPnPEstimator(K=c.K, hypotheses=c.H, threshold_px=c.threshold_px, refine_iters=c.refine_iters, seed=c.seed,
                                solver=solver)


def _compare(r, rep, label, used):
    """One device result against the restatement's report of the case (tests/p3p_cases.py). Exact-set cases: every integer
    field and the mask equal, R, t and rms_px within 10 * GAP of the extended run, GAP being the fp64 restatement's own
    distance from that run for the case (tools/p3p_gap.py prints the table). Other cases: every decision outside the band
    equal."""
    c, ref, ext = rep["case"], rep["ref"], rep["ext"]
    assert r["n_corr"] == c.n, label
    if rep["exact"]:
        for k in ("valid", "best_hypothesis", "iterations", "refined", "n_inliers"):
            assert r[k] == ref[k], (label, k, r[k], ref[k])
        assert r["mask"].tobytes() == ref["mask"].tobytes(), label
        if not ref["valid"]:
            assert np.array_equal(r["R"], np.eye(3)) and not r["t"].any() and r["rms_px"] == 0.0, label
            return
        gap = QC.gap(c)
        dR, dt, drms = QC.diff(r, ext)
        print("%s: R %.2e (allowed %.2e)  t %.2e (allowed %.2e)  rms_px %.2e (allowed %.2e)" %
              (label, dR, 10 * gap[0], dt, 10 * gap[1], drms, 10 * gap[2]))
        used.append(tuple(d / (10 * g) if g > 0 else 0.0 for d, g in zip((dR, dt, drms), gap)))
        assert dR <= 10 * gap[0] and dt <= 10 * gap[1] and drms <= 10 * gap[2], label
        return
    soft = rep["in_band"]
    assert r["valid"] == ref["valid"] == 1 and r["best_hypothesis"] == ref["best_hypothesis"], label
    assert abs(r["n_inliers"] - ref["n_inliers"]) <= soft, label
    assert not ((r["mask"] != ref["mask"]) & ~rep["soft"]).any(), label
    if ref["refit_R"] is not None and abs(ref["n_refit"] - ref["n_winner"]) > soft:
        assert r["refined"] == ref["refined"], label


@pytest.mark.parametrize("i", range(len(QC.P3P_CASES)), ids=lambda i: QC.case_id(QC.P3P_CASES[i]))
def test_whole_stage_equals_the_restatement(aria, i):
    """aria_pnp_estimate with the P3P solver against pnp_ref.estimate(solver="p3p") on every case of the table: counts 0, 3
    (valid = 0), 4, 5 (valid, no refinement), 6, 40 at 30 and 50 % outliers, four planar scenes, a collinear scene, copies
    (none valid; a tie scene won by hypothesis 1), a world origin 1000 units away, no refinement, 2049 across the scoring
    tile; H = 64, 320, 1024; three seeds; pair ids up to 1 000 000; both cameras; thresholds 0.5 / 2 / 8 px.

    Tolerance: measured, not chosen -- 10 * GAP against the restatement's np.longdouble run, the rule of the DLT table. What
    the device showed is in DESIGN.md section 24."""
    c = QC.P3P_CASES[i]
    rep = QC.report(c)
    e = _estimator(aria, c)
    try:
        assert e.solver == "p3p"
        r = e.estimate(rep["corr"], c.pair_base)
    finally:
        e.close()
    used = []
    _compare(r, rep, "case %d (%s)" % (i, QC.case_id(c)), used)
    if used:
        print("case %d share of the allowance used: R %.2f t %.2f rms_px %.2f" % ((i,) + used[0]))


def _pack(torch, corrs, cap, dev):
    B = len(corrs)
    cc = np.zeros((B, cap, CORR), np.uint8)
    nc = np.zeros(B, np.int32)
    for p, c in enumerate(corrs):
        cc[p, :len(c)] = np.ascontiguousarray(c).view(np.uint8).reshape(-1, CORR)
        nc[p] = len(c)
    return torch.from_numpy(cc).to(dev), torch.from_numpy(nc).to(dev)


def _run_batch(est, bufs, cap, lo, hi, pair_base, out, mask):
    cc, nc = bufs
    est.estimate_batch_device(cc.data_ptr() + lo * cap * CORR, nc.data_ptr() + lo * 4, hi - lo, cap, out.data_ptr() + lo * REC,
                              mask.data_ptr() + lo * cap, pair_base)


def test_batch_launch_equals_the_restatement(aria, torch_cuda):
    """aria_pnp_estimate_batch_device with the P3P solver, one launch over QC.P3P_BATCH: 300, 0, 3, 4, 2047, 5, 2048, 6, 40 and
    150 correspondences side by side, each pair against pnp_ref.estimate(solver="p3p") with its own pair id."""
    torch = torch_cuda
    dev = torch.device("cuda", 0)
    cases = QC.P3P_BATCH
    cap = max(c.n for c in cases)
    bufs = _pack(torch, [QC.report(c)["corr"] for c in cases], cap, dev)
    out = torch.zeros(len(cases) * REC, dtype=torch.uint8, device=dev)
    mask = torch.full((len(cases) * cap,), 7, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    e = _estimator(aria, cases[0])
    try:
        _run_batch(e, bufs, cap, 0, len(cases), QC.BATCH_BASE, out, mask)
        e.check()
    finally:
        e.close()
    rec = np.frombuffer(out.cpu().numpy().tobytes(), aria._lib.PNP_RESULT_DTYPE)
    mk = mask.cpu().numpy().reshape(len(cases), cap)
    from aria_slam_amd.pnp import _result_dict
    used = []
    for p, c in enumerate(cases):
        assert not mk[p, c.n:].any(), p
        _compare(_result_dict(rec[p], mk[p, :c.n].copy()), QC.report(c), "pair %d (%s)" % (p, QC.case_id(c)), used)
    print("batch: worst share of the allowance used: R %.2f t %.2f rms_px %.2f" % tuple(np.max(np.array(used), axis=0)))


@pytest.mark.parametrize("i", [6, 8, 14, 16])
def test_hypotheses_against_the_restatement(aria, i):
    """aria_pnp_debug_hypotheses with the P3P solver on four cases (40 correspondences at 50 % outliers and 1024 hypotheses, a
    planar scene at 30 % outliers, the far origin, 2049 correspondences): the sample indices are the restatement's exactly,
    slots 4 and 5 are -1; validity agrees on at least 99 % of the hypotheses (a sample at a double root may branch
    differently); at least 99 % of the agreeing hypotheses hold the same pose to fp32 rounding, and every agreeing
    hypothesis's count equals the restatement's up to that hypothesis's in-band points. Measured: validity agreed on every
    hypothesis of the four cases (1728), and every pose valid on both sides was bit-identical."""
    from aria_slam_amd import pnp_ref as N
    c = QC.P3P_CASES[i]
    rep = QC.report(c)
    e = _estimator(aria, c)
    try:
        idx, R, t0, cnt = e.debug_hypotheses(rep["corr"], c.pair_base)
    finally:
        e.close()
    ridx, rR, rt0, rcnt = rep["hyp"]
    assert idx.shape == (c.H, 6) and np.array_equal(idx, ridx) and (idx[:, 4:] == -1).all() and (idx[:, :4] >= 0).all()
    both = (cnt >= 0) & (rcnt >= 0)
    agree = ((cnt >= 0) == (rcnt >= 0)).mean()
    st = rep["staged"]
    thr2 = N.threshold2(c.threshold_px, c.K)
    rows = np.flatnonzero(both)
    scale = np.maximum(1.0, np.abs(rt0[rows]).max(axis=1))
    same_pose = (np.abs(R[rows] - rR[rows]).max(axis=1) < 1e-5) & (np.abs(t0[rows] - rt0[rows]).max(axis=1) / scale < 1e-5)
    print("case %d: validity agrees on %.4f of %d hypotheses, %d valid on both sides, %d of them with the same pose, "
          "%d bit-identical" % (i, agree, c.H, both.sum(), same_pose.sum(),
                                int(((R[rows] == rR[rows]).all(axis=1) & (t0[rows] == rt0[rows]).all(axis=1)).sum())))
    assert agree >= 0.99 and both.sum() > 0.5 * c.H
    assert same_pose.mean() >= 0.99
    for a in range(0, len(rows), 256):
        sel = rows[a:a + 256]
        near = (np.abs(N.error_ratio(rR[sel], rt0[sel], st["d32"], st["xy32"], thr2) - 1.0) < QC.BAND).sum(axis=1)
        assert (np.abs(cnt[sel] - rcnt[sel]) <= near).all()


def test_planar_scenes_yield_a_pose_where_the_default_solver_yields_none(aria):
    """The planar cases of the table (150 correspondences on one plane, 0 and 30 % outliers, two motions, both cameras): with
    the P3P solver valid = 1 and the pose within twice the restatement's own worst ground-truth error over these cases
    (QC.PLANAR_TRUTH_ERROR: measured on the CPU, printed by tools/p3p_gap.py, pinned by tests/test_p3p_host.py); a handle left
    at the default solver yields valid = 0 on the same input."""
    worst = [0.0, 0.0]
    for i in QC.PLANAR_CASES:
        c = QC.P3P_CASES[i]
        rep = QC.report(c)
        e = _estimator(aria, c)
        d = _estimator(aria, c, solver="dlt")
        try:
            r = e.estimate(rep["corr"], c.pair_base)
            rd = d.estimate(rep["corr"], c.pair_base)
            assert d.solver == "dlt"
        finally:
            e.close()
            d.close()
        assert rd["valid"] == 0 and rd["n_inliers"] == 0 and rd["best_hypothesis"] == -1, i
        assert r["valid"] == 1 and r["n_inliers"] > 10, (i, r["n_inliers"])
        rot, tr, prec = QC.truth_error(r, rep)
        worst = [max(worst[0], rot), max(worst[1], tr)]
        assert rot <= 2 * QC.PLANAR_TRUTH_ERROR[0] and tr <= 2 * QC.PLANAR_TRUTH_ERROR[1], (i, rot, tr)
    print("device worst over the planar cases: rotation %.4f deg, translation %.5f" % tuple(worst))


def test_switching_solvers_on_one_handle(aria):
    """One handle goes DLT, P3P, DLT: the first and the third result are byte-identical and equal a fresh DLT handle's, the
    second equals a fresh P3P handle's; an unknown solver value is refused and changes nothing."""
    from aria_slam_amd import pnp_ref as N
    R, t = PC.motion(2)
    corr = N.synth_pnp(61, 200, R, t, 0.3)[0]
    e = aria.HipPnPEstimator(hypotheses=320)
    fresh_d = aria.HipPnPEstimator(hypotheses=320)
    fresh_p = aria.HipPnPEstimator(hypotheses=320, solver="p3p")
    try:
        assert e.solver == "dlt"
        a = e.estimate(corr, 9)
        e.solver = "p3p"
        assert e.solver == "p3p"
        b = e.estimate(corr, 9)
        for bad in (2, -1, 1 << 20):
            assert e.set_solver_code(bad) == E_INVALID and e.solver == "p3p"
        b2 = e.estimate(corr, 9)
        e.solver = "dlt"
        c = e.estimate(corr, 9)
        want_d, want_p = fresh_d.estimate(corr, 9), fresh_p.estimate(corr, 9)
        with pytest.raises(ValueError):
            e.solver = "epnp"
        assert e.solver == "dlt"
    finally:
        e.close()
        fresh_d.close()
        fresh_p.close()
    assert a["record"] == c["record"] == want_d["record"] and np.array_equal(a["mask"], c["mask"]) and np.array_equal(a["mask"], want_d["mask"])
    assert b["record"] == b2["record"] == want_p["record"] and np.array_equal(b["mask"], want_p["mask"])
    assert a["valid"] == 1 and b["valid"] == 1 and a["record"] != b["record"]


def _varied(n_pairs):
    from aria_slam_amd import pnp_ref as N
    rng = np.random.default_rng(4)
    out = []
    for p in range(n_pairs):
        n = int(rng.choice([0, 3, 4, 5, 6, 12, 40, 150, 300, 600]))
        R, t = PC.motion(p)
        corr = N.synth_pnp(500 + p, max(n, 1), R, t, 0.3, planar=bool(p % 2))[0]
        out.append(corr[:n])
    return out


def test_batch_equals_single_and_is_deterministic(aria, est, torch_cuda):
    torch = torch_cuda
    dev = torch.device("cuda", 0)
    P_, cap, base = 32, 600, 100
    corrs = _varied(P_)
    bufs = _pack(torch, corrs, cap, dev)
    torch.cuda.synchronize()                       # the handle's own stream is not ordered against torch's default stream
    runs = []
    for split in ((0, 32), (0, 11, 32), (0, 32)):
        out = torch.zeros(P_ * REC, dtype=torch.uint8, device=dev)
        mask = torch.full((P_ * cap,), 7, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        for a, b in zip(split[:-1], split[1:]):
            _run_batch(est, bufs, cap, a, b, base + a, out, mask)
        est.check()
        runs.append((out.cpu().numpy().tobytes(), mask.cpu().numpy()))
    assert runs[0][0] == runs[2][0] and np.array_equal(runs[0][1], runs[2][1])     # run to run
    assert runs[0][0] == runs[1][0] and np.array_equal(runs[0][1], runs[1][1])     # split batch
    rec, mask = runs[0]
    n_valid = 0
    for p, c in enumerate(corrs):
        r = est.estimate(c, base + p)
        assert rec[p * REC:(p + 1) * REC] == r["record"], p
        assert np.array_equal(mask[p * cap:p * cap + len(c)], r["mask"]) and not mask[p * cap + len(c):(p + 1) * cap].any()
        assert r["valid"] == (1 if len(c) >= 4 else 0), (p, len(c))
        n_valid += r["valid"]
    assert n_valid > P_ // 2


def _all_finite(record):
    return bool(np.isfinite(np.frombuffer(record[:104], np.float64)).all())


def test_edges(aria, est, torch_cuda):
    from aria_slam_amd import pnp_ref as N
    R, t = PC.motion(1)
    corr = N.synth_pnp(9, 300, R, t, 0.2)[0]
    for n in (0, 3):
        r = est.estimate(corr[:n])
        assert r["valid"] == 0 and not r["mask"].any() and np.array_equal(r["R"], np.eye(3)) and not r["t"].any()
        assert r["best_hypothesis"] == -1 and r["n_corr"] == n and r["n_inliers"] == 0 and r["rms_px"] == 0.0
    # a bad count in the middle pair of three: reported once, skipped before any read, neighbours untouched
    torch = torch_cuda
    dev = torch.device("cuda", 0)
    corrs = [N.synth_pnp(30 + k, 200, *PC.motion(k), 0.2)[0] for k in range(3)]
    cap = 200
    for bad in (201, -1):
        cc, nc = _pack(torch, corrs, cap, dev)
        nc[1] = bad
        out = torch.zeros(3 * REC, dtype=torch.uint8, device=dev)
        mask = torch.full((3 * cap,), 7, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        _run_batch(est, (cc, nc), cap, 0, 3, 0, out, mask)
        assert est.status() == E_INVALID
        assert est.status() == aria._lib.ARIA_OK                                # reported once
        o = out.cpu().numpy().tobytes()
        mh = mask.cpu().numpy()
        for p in (0, 2):
            w = est.estimate(corrs[p], p)
            assert o[p * REC:(p + 1) * REC] == w["record"] and np.array_equal(mh[p * cap:(p + 1) * cap], w["mask"])
        rec1 = np.frombuffer(o[REC:2 * REC], aria._lib.PNP_RESULT_DTYPE)[0]
        assert rec1["valid"] == 0 and rec1["n_corr"] == 0 and rec1["best_hypothesis"] == -1 and not mh[cap:2 * cap].any()
    # NaN / Inf / 3e38 inputs leave every field finite, and the clean correspondences still carry the pose
    rng = np.random.default_rng(1)
    for fill in (np.nan, np.inf, -np.inf, 3e38):
        dirty = corr.copy()
        rows = 1 + rng.permutation(299)[:60]                     # correspondence 0 carries X0: see below
        dirty["X"][rows[:20], rng.integers(0, 3, 20)] = fill
        dirty["u"][rows[20:40]] = fill
        dirty["v"][rows[40:]] = fill
        r = est.estimate(dirty)
        assert _all_finite(r["record"]), fill
        assert r["valid"] == 1 and not r["mask"][rows].any() and N.rotation_error_deg(r["R"], R) < 2 * 0.6548, fill   # the DLT table's bound
        first = corr.copy()
        first["X"][0] = fill                         # X0 itself: nothing can be centred
        r = est.estimate(first)
        assert _all_finite(r["record"]) and r["n_corr"] == 300, fill
        everything = corr.copy()
        everything["X"][:] = fill
        everything["u"][:] = fill
        r = est.estimate(everything)
        assert _all_finite(r["record"]) and r["valid"] == 0 and not r["mask"].any(), fill


def test_device_chain_map_associate_pose(aria, est, torch_cuda):
    """tests/test_gpu_pnp.py::test_device_chain_map_associate_pose's scene with the P3P solver: views 1 and 2 triangulated into
    the map on the device, view 3's matches joined with it and view 3 placed, on one stream; the association does not depend
    on the solver, and the pose record equals the host form's on the fetched correspondences byte for byte."""
    from aria_slam_amd import _lib
    from aria_slam_amd import pnp_ref as N
    from aria_slam_amd import pose_ref as P
    from test_gpu_pnp import _project
    torch = torch_cuda
    dev = torch.device("cuda", 0)
    K = P.EUROC_K
    rng = np.random.default_rng(77)
    n = 400
    u, v, z = rng.uniform(60, 690, n), rng.uniform(40, 440, n), rng.uniform(3, 12, n)
    X = np.stack([(u - K[2]) / K[0] * z, (v - K[3]) / K[1] * z, z], axis=1)
    R2, t2 = P.rot([0, 1, 0], 4), np.array([1.0, 0.0, 0.0])
    R3, t3 = P.rot([0.1, 1, 0], 7), np.array([1.7, 0.1, 0.4])
    px = [_project(X, np.eye(3), np.zeros(3), K) + rng.normal(0, 0.3, (n, 2)), _project(X, R2, t2, K) + rng.normal(0, 0.3, (n, 2)),
          _project(X, R3, t3, K) + rng.normal(0, 0.3, (n, 2))]
    perm2, perm3 = rng.permutation(n), rng.permutation(n)
    kps = []
    for pts, perm in ((px[0], np.arange(n)), (px[1], perm2), (px[2], perm3)):
        k = np.zeros(n, _lib.KP_DTYPE)
        k["x"][perm], k["y"][perm] = pts[:, 0], pts[:, 1]
        k["size"], k["response"] = 31.0, 1.0
        kps.append(k)
    m12 = np.zeros(300, _lib.MATCH_DTYPE)
    m12["query_idx"] = np.arange(300)
    m12["train_idx"] = perm2[:300]
    m32 = np.zeros(n, _lib.MATCH_DTYPE)
    order = rng.permutation(n)
    m32["query_idx"] = perm3[order]
    m32["train_idx"] = perm2[order]
    wrong = rng.permutation(n)[:60]
    m32["query_idx"][wrong] = perm3[order[np.roll(wrong, 1)]]
    pose = np.zeros(1, _lib.POSE_RESULT_DTYPE)
    pose["R"][0], pose["t"][0], pose["valid"], pose["n_inliers"], pose["n_pose_inliers"], pose["n_matches"] = R2.ravel(), t2, 1, 300, 300, 300
    work = torch.cuda.Stream(device=dev)
    mp = aria.HipMapper(stream=work.cuda_stream)
    pe = aria.HipPnPEstimator(stream=work.cuda_stream, solver="p3p")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)   # noqa: E731
    try:
        with torch.cuda.stream(work):
            d_k1, d_k2, d_pose, d_m12 = up(kps[0]), up(kps[1]), up(pose), up(m12)
            d_k3, d_m32 = up(kps[2]), up(m32)
            d_n = up(np.array([n], np.int32))
            d_n12 = up(np.array([300], np.int32))
            d_corr = torch.zeros(n * CORR, dtype=torch.uint8, device=dev)
            d_ncorr = torch.full((1,), -7, dtype=torch.int32, device=dev)
            d_out = torch.zeros(REC, dtype=torch.uint8, device=dev)
            d_mask = torch.full((n,), 7, dtype=torch.uint8, device=dev)
        work.synchronize()
        mp.triangulate_batch_device(d_k1, d_n, d_k2, d_n, n, d_m12, d_n12, 1, 300, d_pose=d_pose, query_is_first=True, pair_base=11)
        pe.associate_batch_device(mp, 11, 2, d_k3, d_n, n, d_m32, d_n, 1, n, d_corr, d_ncorr)
        pe.estimate_batch_device(d_corr, d_ncorr, 1, n, d_out, d_mask, pair_base=40)
        mp.check()
        pe.check()
        points = mp.read()
        ncorr = int(d_ncorr.cpu().numpy()[0])
        corr = np.frombuffer(d_corr.cpu().numpy().tobytes(), _lib.PNP_CORR_DTYPE)
        rec = d_out.cpu().numpy().tobytes()
        mask = d_mask.cpu().numpy()
    finally:
        pe.close()
        mp.close()
    want_corr, _back = N.associate(points, 11, 2, kps[2], m32)
    assert ncorr == len(want_corr) and 200 <= ncorr < n and corr[:ncorr].tobytes() == want_corr.tobytes()
    host = est.estimate(want_corr, 40)
    assert rec == host["record"] and np.array_equal(mask[:ncorr], host["mask"]) and not mask[ncorr:].any()
    assert host["valid"] == 1 and host["n_inliers"] > 0.7 * ncorr
    want = N.estimate(want_corr, pair=40, solver="p3p")
    assert host["best_hypothesis"] == want["best_hypothesis"] and host["n_inliers"] == want["n_inliers"]
    assert N.rotation_error_deg(host["R"], R3) <= 2 * 0.6548 and np.linalg.norm(host["t"] - t3) <= 2 * 0.17379   # the DLT stage's bound


def test_cpp_p3p_selftest(aria):
    """The C++ adapters with the P3P solver (tests/cpp/p3p_selftest.cpp). HipPnPEstimator::setSolver on a planar scene of 400
    correspondences with 20 % outliers: a pose within twice the restatement's planar ground-truth error
    (QC.PLANAR_TRUTH_ERROR, measured at 150 correspondences and 0.5 px; this scene has more points and 0.3 px), where the
    default solver on the same handle found none; four correspondences give a pose, three none; an unknown solver value
    throws and changes nothing. MapTracker with the P3P option on pnp_selftest.cpp's three-frame 3-D sequence, under that
    test's bounds (tests/test_gpu_pnp.py::test_cpp_pnp_selftest: the ground-truth bounds of the DLT table, 2 * 0.6548 deg and
    2 * 0.17379 map units, the latter carried over to the step ratio). A third frame whose matches are restricted to the
    mapped points of one wall, with no two-view pose offered, is placed by PnP with P3P; what the DLT does there is printed,
    not asserted: triangulated points are only nearly coplanar."""
    subprocess.check_call(["make", "-C", os.path.join(PKG, "host"), "-s"])
    src = os.path.join(ROOT, "tests", "cpp", "p3p_selftest.cpp")
    exe = os.path.join(ROOT, "build", "p3p_selftest")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "host", "include"),
                           src, "-o", exe, "-L" + PKG, "-laria_hip_adapters", "-laria_orb_hip", "-lz", "-Wl,-rpath," + PKG])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "DONE" in out.stdout, out.stdout + out.stderr
    print(out.stdout)
    kv = {l.split()[0]: l.split()[1:] for l in out.stdout.splitlines() if l.strip()}
    pl = kv["planar"]
    assert pl[0] == "1" and pl[5] == "0" and pl[6] == "1"                      # P3P: a pose; the DLT before it: none
    assert float(pl[1]) <= 2 * QC.PLANAR_TRUTH_ERROR[0] and float(pl[2]) <= 2 * QC.PLANAR_TRUTH_ERROR[1] and int(pl[3]) > 250
    assert kv["few"] == ["1", "0"] and kv["unknown"] == ["1", "1"]
    BOOTSTRAP, PNP = "1", "2"
    gt_rot, gt_t = 2 * 0.6548, 2 * 0.17379
    tr = kv["track"]
    assert tr[0] == PNP and tr[8] == BOOTSTRAP and abs(float(tr[7]) - 1.0) < 1e-9   # the first step: one map unit
    assert abs(float(tr[1]) - float(tr[2])) <= gt_t, tr
    assert float(tr[3]) <= gt_rot and float(tr[4]) <= gt_t and int(tr[5]) > 0.7 * int(tr[6])
    wall = kv["wall_p3p"]
    assert int(kv["wall_points"][0]) > 100 and wall[8] == BOOTSTRAP
    assert wall[0] == PNP and int(wall[5]) > 10, wall
    print("wall, DLT (not asserted): source %s inliers %s of %s" % (kv["wall_dlt"][0], kv["wall_dlt"][5], kv["wall_dlt"][6]))


def test_euroc_frontend_pnp_solver_flag(aria, tmp_path):
    """--pnp-solver on the synthetic image sequence (a 2-D shift of a flat scene): with dlt the --track-map and --pose files
    are byte-identical to a run without the flag; with p3p one well-formed TUM line per frame, every step accounted for and
    --pose byte-identical. Whether PnP places a frame there is printed, not asserted: the bootstrap is the 8-point two-view
    stage on a flat scene, and what it leaves in the map is not known. Measured: 1 bootstrap, 4 fallbacks, 6 held steps and 0
    by PnP with either solver."""
    from test_frontend_io import _make_dataset
    subprocess.check_call(["make", "-C", os.path.join(PKG, "host"), "-s"])
    _make_dataset(aria, str(tmp_path), 6, w=640, h=480)          # 6 synthetic pairs
    exe = os.path.join(PKG, "euroc_frontend")
    runs = {}
    for name, extra in (("plain", []), ("dlt", ["--pnp-solver", "dlt"]), ("p3p", ["--pnp-solver", "p3p"])):
        pose, tm = str(tmp_path / (name + "_pose.txt")), str(tmp_path / (name + "_track.txt"))
        run = subprocess.run([exe, str(tmp_path), "1000", "--pose", pose, "--track-map", tm] + extra, capture_output=True, text=True, timeout=300)
        assert run.returncode == 0, run.stdout + run.stderr
        line = [l.split() for l in run.stdout.splitlines() if l.startswith("track ")]
        assert len(line) == 1, run.stdout
        w = line[0]
        runs[name] = dict(pose=open(pose, "rb").read(), track=open(tm, "rb").read(),
                          counts=dict(pnp=int(w[2]), fallback=int(w[4]), bootstrap=int(w[6]), held=int(w[8])))
        print(name, " ".join(w[:9]))
    assert runs["plain"]["pose"] == runs["dlt"]["pose"] == runs["p3p"]["pose"]
    assert runs["plain"]["track"] == runs["dlt"]["track"] and runs["plain"]["counts"] == runs["dlt"]["counts"]
    n_frames = len(runs["plain"]["pose"].splitlines())
    assert n_frames == 12
    rows = [l.split() for l in runs["p3p"]["track"].decode().splitlines()]
    assert len(rows) == n_frames and all(len(r) == 8 and all(np.isfinite(float(x)) for x in r) for r in rows)
    assert [float(x) for x in rows[0][1:]] == [0, 0, 0, 0, 0, 0, 1]
    c = runs["p3p"]["counts"]
    assert sum(c.values()) == n_frames - 1 and c["bootstrap"] <= 1
    bad = subprocess.run([exe, str(tmp_path), "1000", "--pose", str(tmp_path / "x.txt"), "--pnp-solver", "epnp"], capture_output=True, text=True, timeout=60)
    assert bad.returncode != 0 and "--pnp-solver" in bad.stderr
