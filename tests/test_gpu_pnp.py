"""Absolute pose from the point map on the MI355X (aria_pnp_*, kernels in aria_slam_amd/csrc/pnp_ransac.hip): hypotheses against
the NumPy restatement, the whole stage against it over the case table of tests/pnp_cases.py, batch == single and determinism,
edge cases, ground-truth accuracy and the device chain map -> association -> pose. The reference project has no PnP code:
aria_slam_amd/pnp_ref.py is the definition."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pnp_cases as PC   # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "aria_slam_amd")
REC = 128                                                    # bytes of an aria_pnp_result
CORR = 32                                                    # bytes of an aria_pnp_corr

# The restatement's worst error against ground truth over PC.GT_CASES, measured on the CPU (tools/pnp_gap.py; pinned by
# tests/test_pnp_host.py): rotation 0.6548 deg, |t - t_true| 0.17379, mask precision 1.0. The device is allowed twice that.
GT_WORST = (0.6548, 0.17379, 1.0)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def est(aria):
    e = aria.HipPnPEstimator()
    yield e
    e.close()


def _estimator(aria, c):
    return aria.HipPnPEstimator(K=c.K, hypotheses=c.H, threshold_px=c.threshold_px, refine_iters=c.refine_iters, seed=c.seed)


@pytest.mark.parametrize("i", [9, 16, 17, 18, 19])
def test_hypotheses_against_the_restatement(aria, i):
    """aria_pnp_debug_hypotheses on five cases of the table (600, 2049 and 4096 correspondences, 320 to 4096 hypotheses, the
    far origin): the sample indices are the restatement's exactly; validity agrees on more than 99 % of the hypotheses; the
    poses agree to fp32 rounding; each count equals the restatement's up to that hypothesis's in-band points."""
    from aria_slam_amd import pnp_ref as N
    c = PC.PNP_CASES[i]
    rep = PC.report(c)
    e = _estimator(aria, c)
    try:
        idx, R, t0, cnt = e.debug_hypotheses(rep["corr"], c.pair_base)
    finally:
        e.close()
    ridx, rR, rt0, rcnt = rep["hyp"]
    assert idx.shape == (c.H, 6) and np.array_equal(idx, ridx)
    both = (cnt >= 0) & (rcnt >= 0)
    agree = ((cnt >= 0) == (rcnt >= 0)).mean()
    print("case %d: validity agrees on %.4f of %d hypotheses, %d valid on both sides" % (i, agree, c.H, both.sum()))
    assert agree > 0.99 and both.sum() > 0.5 * c.H
    scale = np.maximum(1.0, np.abs(rt0[both]).max(axis=1, keepdims=True))
    assert np.abs(R[both] - rR[both]).max() < 1e-5 and (np.abs(t0[both] - rt0[both]) / scale).max() < 1e-5
    st = rep["staged"]
    thr2 = N.threshold2(c.threshold_px, c.K)
    rows = np.flatnonzero(both)
    for a in range(0, len(rows), 256):
        sel = rows[a:a + 256]
        near = (np.abs(N.error_ratio(rR[sel], rt0[sel], st["d32"], st["xy32"], thr2) - 1.0) < PC.BAND).sum(axis=1)
        assert (np.abs(cnt[sel] - rcnt[sel]) <= near).all()
    if c.n > PC.TILE:                                      # the counts reach past the first LDS tile
        beyond = N.inliers32(rR[rows[:64]], rt0[rows[:64]], st["d32"][PC.TILE:], st["xy32"][PC.TILE:], thr2).sum(axis=1)
        assert (beyond > 0).sum() >= 5


# ---- the whole stage against pnp_ref.estimate over the case table (tests/pnp_cases.py) -----------------------------------
# GAP, measured on the CPU with the committed restatement (tools/pnp_gap.py prints these tables): per exact-set case, the
# largest difference of R, t and rms_px between pnp_ref's fp64 run and its np.longdouble run.
PNP_GAP = {    # case: (R, t, rms_px)
     0: (8.48e-16, 5.41e-15, 1.33e-14),    # s1-n6-H64
     1: (4.54e-16, 1.25e-15, 8.39e-15),    # s2-n7-H64
     2: (3.63e-16, 3.61e-15, 1.40e-14),    # s3-n7-H1024
     3: (2.59e-16, 1.23e-15, 8.19e-15),    # s4-n40-H320
     4: (7.79e-16, 3.89e-15, 1.49e-14),    # s5-n40-H64
     5: (7.29e-16, 5.34e-16, 9.02e-15),    # s6-n40-H1024
     6: (3.42e-16, 5.62e-16, 6.43e-15),    # s7-n150-H320
     8: (2.62e-16, 2.94e-15, 2.69e-15),    # s9-n600-H320
     9: (1.73e-16, 1.14e-15, 1.57e-15),    # s280-n600-H1024
    10: (4.02e-16, 5.54e-15, 2.72e-14),    # s11-n600-H64
    11: (2.66e-16, 8.74e-16, 7.13e-16),    # s12-n2047-H320
    12: (3.78e-16, 8.64e-16, 5.60e-16),    # s13-n2047-H64
    13: (3.25e-16, 8.19e-16, 2.07e-15),    # s14-n2048-H320
    14: (6.88e-16, 4.90e-15, 3.43e-15),    # s381-n2048-H64
    15: (2.44e-16, 1.03e-15, 3.22e-16),    # s400-n2049-H64
    16: (5.74e-16, 3.02e-15, 6.22e-15),    # s421-n2049-H320
    17: (2.40e-16, 3.25e-16, 3.42e-16),    # s446-n4096-H320
    18: (2.65e-16, 1.74e-15, 5.27e-15),    # s19-n300-H4096
    19: (6.13e-16, 5.99e-13, 5.44e-14),    # s20-n600-H320, origin at 1000
    20: (0.00e+00, 1.02e-15, 3.22e-15),    # s21-n150-H320, no refinement
    23: (5.47e-16, 1.74e-15, 3.15e-15),    # s24-n150-H1024, tie
    24: (5.37e-16, 7.91e-16, 4.16e-15),    # s24-n150-H1024, tie
}
PNP_BATCH_GAP = {    # pair: (R, t, rms_px)
     0: (3.44e-16, 1.05e-15, 2.88e-15),    # s200-n300
     2: (3.23e-16, 6.28e-16, 1.40e-15),    # s202-n2047
     4: (2.87e-16, 3.70e-16, 1.53e-15),    # s204-n2048
     5: (3.18e-16, 3.07e-16, 4.43e-15),    # s205-n6
     6: (7.36e-16, 1.34e-15, 1.38e-15),    # s206-n2049
     7: (3.17e-16, 1.29e-15, 1.72e-14),    # s207-n40
     8: (1.89e-16, 1.13e-15, 1.54e-15),    # s228-n600
    10: (4.23e-16, 2.22e-15, 5.58e-15),    # s210-n150
}


def _compare(r, rep, gap, label):
    """One device result against the restatement's report of the case (tests/pnp_cases.py). Exact-set cases: every integer
    field and the mask equal, R, t and rms_px within 10 * GAP of the extended run. Other cases: the winner equal, the counts
    within the in-band points, the mask different only at those points."""
    c, ref, ext = rep["case"], rep["ref"], rep["ext"]
    assert r["n_corr"] == c.n, label
    if rep["exact"]:
        for k in ("valid", "best_hypothesis", "iterations", "refined", "n_inliers"):
            assert r[k] == ref[k], (label, k, r[k], ref[k])
        assert r["mask"].tobytes() == ref["mask"].tobytes(), label
        if not ref["valid"]:
            assert np.array_equal(r["R"], np.eye(3)) and not r["t"].any() and r["rms_px"] == 0.0, label
            return
        dR, dt, drms = PC.diff(r, ext)
        print("%s: R %.2e (allowed %.2e)  t %.2e (allowed %.2e)  rms_px %.2e (allowed %.2e)" %
              (label, dR, 10 * gap[0], dt, 10 * gap[1], drms, 10 * gap[2]))
        assert dR <= 10 * gap[0] and dt <= 10 * gap[1] and drms <= 10 * gap[2], label
        return
    soft = rep["in_band"]
    assert r["valid"] == ref["valid"] == 1 and r["best_hypothesis"] == ref["best_hypothesis"], label
    assert abs(r["n_inliers"] - ref["n_inliers"]) <= soft, label
    assert not ((r["mask"] != ref["mask"]) & ~rep["soft"]).any(), label
    if ref["refit_R"] is not None and abs(ref["n_refit"] - ref["n_winner"]) > soft:
        assert r["refined"] == ref["refined"], label
    print("%s: not exact-set (%d in-band): n_inliers %d / %d, mask differs at %d" %
          (label, rep["in_band"], r["n_inliers"], ref["n_inliers"], int((r["mask"] != ref["mask"]).sum())))


@pytest.mark.parametrize("i", range(len(PC.PNP_CASES)), ids=lambda i: PC.case_id(PC.PNP_CASES[i]))
def test_whole_stage_equals_the_restatement(aria, i):
    """aria_pnp_estimate against pnp_ref.estimate on every case of the table: counts at the gate (6, 7), mid sizes, around
    the 2048-point tile and 4096; H = 64, 320, 1024, 4096; seeds 0, 3 and one with the top bit set; pair ids 0, 5, 1 000 000;
    thresholds 0.5 / 2 / 8 px; both cameras; outliers 0 to 0.5; a world origin 1000 units away; no refinement; ties won by
    hypotheses 1 and 6; no valid hypothesis; a coplanar scene. tests/test_pnp_host.py proves with the restatement alone that
    every case can be decided and what the table covers.

    Tolerance: measured, not chosen. The device is allowed 10 * GAP against the restatement's np.longdouble run, GAP being
    the fp64 run's own distance from it (PNP_GAP above, tools/pnp_gap.py): one decade for another summation order and
    another 3x3 solver. What the device showed is in DESIGN.md section 24.

    GAP as measured (the case numbers index the table of tests/pnp_cases.py):
        case  n      H      R         t         rms_px
        0     6      64     8.48e-16  5.41e-15  1.33e-14
        1     7      64     4.54e-16  1.25e-15  8.39e-15
        2     7      1024   3.63e-16  3.61e-15  1.40e-14
        3     40     320    2.59e-16  1.23e-15  8.19e-15
        4     40     64     7.79e-16  3.89e-15  1.49e-14
        5     40     1024   7.29e-16  5.34e-16  9.02e-15
        6     150    320    3.42e-16  5.62e-16  6.43e-15
        8     600    320    2.62e-16  2.94e-15  2.69e-15
        9     600    1024   1.73e-16  1.14e-15  1.57e-15
        10    600    64     4.02e-16  5.54e-15  2.72e-14
        11    2047   320    2.66e-16  8.74e-16  7.13e-16
        12    2047   64     3.78e-16  8.64e-16  5.60e-16
        13    2048   320    3.25e-16  8.19e-16  2.07e-15
        14    2048   64     6.88e-16  4.90e-15  3.43e-15
        15    2049   64     2.44e-16  1.03e-15  3.22e-16
        16    2049   320    5.74e-16  3.02e-15  6.22e-15
        17    4096   320    2.40e-16  3.25e-16  3.42e-16
        18    300    4096   2.65e-16  1.74e-15  5.27e-15
        19    600    320    6.13e-16  5.99e-13  5.44e-14
        20    150    320    0.00e+00  1.02e-15  3.22e-15
        23    150    1024   5.47e-16  1.74e-15  3.15e-15
        24    150    1024   5.37e-16  7.91e-16  4.16e-15
    Cases 21 and 22 (no valid hypothesis, coplanar) and 7, 25, 26 (not exact-set) have no row: R, t and rms_px are not
    compared there."""
    c = PC.PNP_CASES[i]
    rep = PC.report(c)
    e = _estimator(aria, c)
    try:
        r = e.estimate(rep["corr"], c.pair_base)
    finally:
        e.close()
    _compare(r, rep, PNP_GAP.get(i), "case %d (%s)" % (i, PC.case_id(c)))


def _pack(torch, corrs, cap, dev):
    """Device blocks for a list of correspondence arrays: pair p at p * cap (32 B each), and the counts."""
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
    """aria_pnp_estimate_batch_device, one launch over PC.PNP_BATCH: 300, 0, 2047, 5, 2048, 6, 2049, 40, 600, 4 and 150
    correspondences side by side, each pair against pnp_ref.estimate with its own pair id (tolerances: PNP_BATCH_GAP).

    GAP as measured (tools/pnp_gap.py prints it; by pair of the launch):
        pair  n      R         t         rms_px
        0     300    3.44e-16  1.05e-15  2.88e-15
        2     2047   3.23e-16  6.28e-16  1.40e-15
        4     2048   2.87e-16  3.70e-16  1.53e-15
        5     6      3.18e-16  3.07e-16  4.43e-15
        6     2049   7.36e-16  1.34e-15  1.38e-15
        7     40     3.17e-16  1.29e-15  1.72e-14
        8     600    1.89e-16  1.13e-15  1.54e-15
        10    150    4.23e-16  2.22e-15  5.58e-15
    """
    torch = torch_cuda
    dev = torch.device("cuda", 0)
    cases = PC.PNP_BATCH
    cap = max(c.n for c in cases)
    bufs = _pack(torch, [PC.report(c)["corr"] for c in cases], cap, dev)
    out = torch.zeros(len(cases) * REC, dtype=torch.uint8, device=dev)
    mask = torch.full((len(cases) * cap,), 7, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    e = _estimator(aria, cases[0])
    try:
        _run_batch(e, bufs, cap, 0, len(cases), PC.BATCH_BASE, out, mask)
        e.check()
    finally:
        e.close()
    rec = np.frombuffer(out.cpu().numpy().tobytes(), aria._lib.PNP_RESULT_DTYPE)
    mk = mask.cpu().numpy().reshape(len(cases), cap)
    from aria_slam_amd.pnp import _result_dict
    for p, c in enumerate(cases):
        assert not mk[p, c.n:].any(), p
        _compare(_result_dict(rec[p], mk[p, :c.n].copy()), PC.report(c), PNP_BATCH_GAP.get(p), "pair %d (%s)" % (p, PC.case_id(c)))


def _varied(n_pairs):
    from aria_slam_amd import pnp_ref as N
    rng = np.random.default_rng(3)
    out = []
    for p in range(n_pairs):
        n = int(rng.choice([0, 5, 6, 12, 40, 150, 300, 600]))
        R, t = PC.motion(p)
        corr = N.synth_pnp(300 + p, max(n, 1), R, t, 0.3)[0]
        out.append(corr[:n])
    return out


def test_batch_equals_single_and_is_deterministic(aria, est, torch_cuda):
    torch = torch_cuda
    dev = torch.device("cuda", 0)
    P_, cap, base = 48, 600, 100
    corrs = _varied(P_)
    bufs = _pack(torch, corrs, cap, dev)
    torch.cuda.synchronize()                       # the handle's own stream is not ordered against torch's default stream
    runs = []
    for split in ((0, 48), (0, 17, 48), (0, 48)):
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
        n_valid += r["valid"]
    assert n_valid > P_ // 2


def _all_finite(record):
    return bool(np.isfinite(np.frombuffer(record[:104], np.float64)).all())


def test_edges(aria, est, torch_cuda):
    from aria_slam_amd import pnp_ref as N
    R, t = PC.motion(1)
    corr = N.synth_pnp(9, 300, R, t, 0.2)[0]
    for n in (0, 5):
        r = est.estimate(corr[:n])
        assert r["valid"] == 0 and not r["mask"].any() and np.array_equal(r["R"], np.eye(3)) and not r["t"].any()
        assert r["best_hypothesis"] == -1 and r["n_corr"] == n and r["n_inliers"] == 0 and r["rms_px"] == 0.0
    six = N.synth_pnp(10, 6, R, t, 0.0, 0.05)[0]
    r = est.estimate(six)
    want = N.estimate(six)
    assert r["valid"] == want["valid"] == 1 and r["n_corr"] == 6 and r["best_hypothesis"] == want["best_hypothesis"]
    assert r["n_inliers"] == want["n_inliers"] and np.array_equal(r["mask"], want["mask"])
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
        assert est.status() == aria._lib.ARIA_OK - 1                            # ARIA_E_INVALID
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
        assert r["valid"] == 1 and not r["mask"][rows].any() and N.rotation_error_deg(r["R"], R) < 2 * GT_WORST[0], fill
        first = corr.copy()
        first["X"][0] = fill                         # X0 itself: nothing can be centred
        r = est.estimate(first)
        assert _all_finite(r["record"]) and r["n_corr"] == 300, fill
        everything = corr.copy()
        everything["X"][:] = fill
        everything["u"][:] = fill
        r = est.estimate(everything)
        assert _all_finite(r["record"]) and r["valid"] == 0 and not r["mask"].any(), fill


def test_ground_truth(aria):
    """The device's pose and mask against the scene's truth over PC.GT_CASES (0.5 px noise, 0 to 50 % outliers, 40 to 4096
    correspondences). Bounds: twice the restatement's own worst error over the same cases, measured on the CPU --
    rotation 0.6548 deg, |t - t_true| 0.17379 units, mask precision 1.0 (tools/pnp_gap.py; tests/test_pnp_host.py pins the
    three numbers)."""
    worst = [0.0, 0.0, 1.0]
    for i in PC.GT_CASES:
        c = PC.PNP_CASES[i]
        rep = PC.report(c)
        e = _estimator(aria, c)
        try:
            r = e.estimate(rep["corr"], c.pair_base)
        finally:
            e.close()
        assert r["valid"] == 1, i
        rot, tr, prec = PC.truth_error(r, rep)
        worst = [max(worst[0], rot), max(worst[1], tr), min(worst[2], prec)]
        assert rot <= 2 * GT_WORST[0] and tr <= 2 * GT_WORST[1] and prec >= 1.0 - 2 * (1.0 - GT_WORST[2]), (i, rot, tr, prec)
    print("device worst over %d cases: rotation %.4f deg, translation %.5f, mask precision %.4f" % ((len(PC.GT_CASES),) + tuple(worst)))


def _project(X, R, t, K):
    fx, fy, cx, cy = K
    Xc = X @ np.asarray(R).T + t
    return np.stack([fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy], axis=1)


def test_device_chain_map_associate_pose(aria, est, torch_cuda):
    """A synthetic 3-D scene seen by three views. Views 1 and 2 are triangulated into the map on the device from a pose record
    (aria_map_triangulate_batch_device); view 3's matches against view 2 are joined with the map
    (aria_pnp_associate_batch_device) and view 3 is placed (aria_pnp_estimate_batch_device), all on one stream with no host
    step between. The association equals pnp_ref.associate on the fetched map -- a view-2 keypoint with two map points takes
    the one at the lowest arena position, a keypoint without a map point yields nothing --, the pose record equals the host
    form on the fetched correspondences byte for byte, and the pose is within the ground-truth bound of the truth. A second
    tracked pair, anchored on a pair id the map does not hold, gets no correspondences."""
    from aria_slam_amd import _lib
    from aria_slam_amd import pnp_ref as N
    from aria_slam_amd import pose_ref as P
    torch = torch_cuda
    dev = torch.device("cuda", 0)
    K = P.EUROC_K
    rng = np.random.default_rng(77)
    n = 400
    u, v, z = rng.uniform(60, 690, n), rng.uniform(40, 440, n), rng.uniform(3, 12, n)
    X = np.stack([(u - K[2]) / K[0] * z, (v - K[3]) / K[1] * z, z], axis=1)
    R2, t2 = P.rot([0, 1, 0], 4), np.array([1.0, 0.0, 0.0])                  # unit baseline, as the E stage would give
    R3, t3 = P.rot([0.1, 1, 0], 7), np.array([1.7, 0.1, 0.4])
    px = [_project(X, np.eye(3), np.zeros(3), K) + rng.normal(0, 0.3, (n, 2)), _project(X, R2, t2, K) + rng.normal(0, 0.3, (n, 2)),
          _project(X, R3, t3, K) + rng.normal(0, 0.3, (n, 2))]
    perm2, perm3 = rng.permutation(n), rng.permutation(n)                    # point i is keypoint perm[i] of its view
    kps = []
    for pts, perm in ((px[0], np.arange(n)), (px[1], perm2), (px[2], perm3)):
        k = np.zeros(n, _lib.KP_DTYPE)
        k["x"][perm], k["y"][perm] = pts[:, 0], pts[:, 1]
        k["size"], k["response"] = 31.0, 1.0
        kps.append(k)
    kps[0]["x"][6], kps[0]["y"][6] = kps[0]["x"][5] + 0.5, kps[0]["y"][5]     # keypoint 6 of view 1: half a pixel from 5
    m12 = np.zeros(300, _lib.MATCH_DTYPE)                                     # points 300.. are not mapped
    m12["query_idx"] = np.arange(300)
    m12["train_idx"] = perm2[:300]
    m12["train_idx"][6] = perm2[5]                                            # two map points on one view-2 keypoint
    m32 = np.zeros(n, _lib.MATCH_DTYPE)
    order = rng.permutation(n)
    m32["query_idx"] = perm3[order]
    m32["train_idx"] = perm2[order]
    wrong = rng.permutation(n)[:60]                                           # 15 % of the matches hit another keypoint
    m32["query_idx"][wrong] = perm3[order[np.roll(wrong, 1)]]
    pose = np.zeros(1, _lib.POSE_RESULT_DTYPE)
    pose["R"][0], pose["t"][0], pose["valid"], pose["n_inliers"], pose["n_pose_inliers"], pose["n_matches"] = R2.ravel(), t2, 1, 300, 300, 300
    work = torch.cuda.Stream(device=dev)
    mp = aria.HipMapper(stream=work.cuda_stream)
    pe = aria.HipPnPEstimator(stream=work.cuda_stream)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)   # noqa: E731
    try:
        with torch.cuda.stream(work):
            d_k1, d_k2, d_pose, d_m12 = up(kps[0]), up(kps[1]), up(pose), up(m12)
            d_k3 = up(np.concatenate([kps[2], kps[2]]))                      # the query side of two tracked pairs
            d_m32 = up(np.concatenate([m32, m32]))
            d_n = up(np.array([n, n], np.int32))
            d_n12 = up(np.array([300], np.int32))
            d_corr = torch.zeros(2 * n * CORR, dtype=torch.uint8, device=dev)
            d_ncorr = torch.full((2,), -7, dtype=torch.int32, device=dev)
            d_back = torch.full((2 * n,), -7, dtype=torch.int32, device=dev)
            d_out = torch.zeros(2 * REC, dtype=torch.uint8, device=dev)
            d_mask = torch.full((2 * n,), 7, dtype=torch.uint8, device=dev)
        work.synchronize()
        mp.triangulate_batch_device(d_k1, d_n, d_k2, d_n, n, d_m12, d_n12, 1, 300, d_pose=d_pose, query_is_first=True, pair_base=11)
        pe.associate_batch_device(mp, 11, 2, d_k3, d_n, n, d_m32, d_n, 2, n, d_corr, d_ncorr, d_back)
        pe.estimate_batch_device(d_corr, d_ncorr, 2, n, d_out, d_mask, pair_base=40)
        mp.check()
        pe.check()
        points = mp.read()
        ncorr = d_ncorr.cpu().numpy()
        corr = np.frombuffer(d_corr.cpu().numpy().tobytes(), _lib.PNP_CORR_DTYPE).reshape(2, n)
        back = d_back.cpu().numpy().reshape(2, n)
        rec = d_out.cpu().numpy().tobytes()
        mask = d_mask.cpu().numpy().reshape(2, n)
    finally:
        pe.close()
        mp.close()
    assert 250 <= len(points) <= 300 and (points["pair"] == 11).all()
    assert ((points["idx2"] == perm2[5]).sum() == 2)                          # the duplicated view-2 keypoint is in the map twice
    want_corr, want_back = N.associate(points, 11, 2, kps[2], m32)
    assert ncorr.tolist() == [len(want_corr), 0] and 200 <= ncorr[0] < n
    assert corr[0, :ncorr[0]].tobytes() == want_corr.tobytes() and np.array_equal(back[0, :ncorr[0]], want_back)
    dup = np.flatnonzero(m32["train_idx"][want_back] == perm2[5])
    assert len(dup) == 1 and np.array_equal(want_corr["X"][dup[0]], points["X"][np.flatnonzero(points["idx2"] == perm2[5])[0]])
    host = est.estimate(want_corr, 40)
    assert rec[:REC] == host["record"] and np.array_equal(mask[0, :ncorr[0]], host["mask"]) and not mask[0, ncorr[0]:].any()
    r1 = np.frombuffer(rec[REC:], _lib.PNP_RESULT_DTYPE)[0]
    assert r1["valid"] == 0 and r1["n_corr"] == 0 and not mask[1].any()
    assert host["valid"] == 1 and host["n_inliers"] > 0.7 * ncorr[0]
    assert N.rotation_error_deg(host["R"], R3) <= 2 * GT_WORST[0] and np.linalg.norm(host["t"] - t3) <= 2 * GT_WORST[1]
    # an out-of-range match index is a deferred error of its pair alone
    bad = m32.copy()
    bad["train_idx"][17] = n
    mp = aria.HipMapper()
    pe = aria.HipPnPEstimator()
    try:
        d_k3, d_m, d_n = up(np.concatenate([kps[2], kps[2]])), up(np.concatenate([bad, m32])), up(np.array([n, n], np.int32))
        d_ncorr = torch.full((2,), -7, dtype=torch.int32, device=dev)
        d_corr = torch.zeros(2 * n * CORR, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        pe.associate_batch_device(mp, 0, 1, d_k3, d_n, n, d_m, d_n, 2, n, d_corr, d_ncorr)
        assert pe.status() == aria._lib.ARIA_OK - 1 and pe.status() == aria._lib.ARIA_OK
        assert d_ncorr.cpu().numpy().tolist() == [0, 0]                       # an empty map: nothing to join
    finally:
        pe.close()
        mp.close()


def test_cpp_pnp_selftest(aria):
    """The C++ adapters: an estimate on a synthetic scene, and MapTracker -- the loop euroc_frontend --track-map runs, with the
    join on the device -- on a three-frame synthetic sequence: frames 0 and 1 bootstrapped by the two-view stage at unit
    baseline (the scene's is 0.5) and triangulated, frame 2 placed by PnP against those points and the new pair triangulated
    with the two extrinsics. One scale: the second step's length over the first is the scene's ratio.

    The bound on the ratio is the ground-truth translation bound, 2 * 0.17379 = 0.348 map units, and the units carry over
    because the first step is exactly one map unit long (the two-view stage's |t| = 1; the test asserts it): an error of the
    third camera's centre of at most 0.348 map units moves the ratio |c2 - c1| / |c1 - c0| by at most 0.348. The map here is the
    scene at twice its size, 6-24 units deep, the depth range the bound was measured at (2-20). Then the fallback rule (no
    mapped keypoint among the matches: the two-view delta is taken, and its pair triangulated) and the held step."""
    import subprocess
    subprocess.check_call(["make", "-C", os.path.join(PKG, "host"), "-s"])
    src = os.path.join(ROOT, "tests", "cpp", "pnp_selftest.cpp")
    exe = os.path.join(ROOT, "build", "pnp_selftest")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "host", "include"),
                           src, "-o", exe, "-L" + PKG, "-laria_hip_adapters", "-laria_orb_hip", "-lz", "-Wl,-rpath," + PKG])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "DONE" in out.stdout, out.stdout + out.stderr
    print(out.stdout)
    kv = {l.split()[0]: l.split()[1:] for l in out.stdout.splitlines() if l.strip()}
    est_ = kv["estimate"]
    assert est_[0] == "1" and float(est_[1]) <= 2 * GT_WORST[0] and float(est_[2]) <= 2 * GT_WORST[1] and int(est_[3]) > 250
    assert kv["too_few"] == ["0"]
    BOOTSTRAP, PNP, FALLBACK, HELD = "1", "2", "3", "0"
    assert kv["bootstrap"][0] == BOOTSTRAP and int(kv["bootstrap"][1]) > 300 and kv["bootstrap"][2] == "0"
    tr = kv["track"]
    assert tr[0] == PNP and abs(float(tr[8]) - 1.0) < 1e-9                    # the first step: one map unit
    assert abs(float(tr[1]) - float(tr[2])) <= 2 * GT_WORST[1], tr
    assert float(tr[3]) <= 2 * GT_WORST[0] and float(tr[4]) <= 2 * GT_WORST[1]
    assert int(tr[6]) == int(kv["bootstrap"][1]) and int(tr[5]) > 0.7 * int(tr[6])   # every mapped keypoint is matched
    assert int(tr[7]) > 300 and int(kv["map"][0]) == int(kv["bootstrap"][1]) + int(tr[7])   # the new pair went into the map
    fb = kv["fallback"]
    assert fb[0] == BOOTSTRAP and fb[1] == FALLBACK and fb[2] == "0" and float(fb[3]) < 1.0 and int(fb[4]) > 100
    assert kv["held"] == [HELD, "0", "1"]


def test_euroc_frontend_track_map(aria, tmp_path):
    """The driver flag on the synthetic image sequence (a 2-D shift of a flat scene): one TUM line per frame, every step
    accounted for, --pose untouched. The scene is planar, the DLT's known limit, so whatever the pose stage accepts is taken
    by the bootstrap and fallback rules and PnP places no frame; what PnP does on a 3-D scene is test_cpp_pnp_selftest's."""
    import subprocess
    from test_frontend_io import _make_dataset
    subprocess.check_call(["make", "-C", os.path.join(PKG, "host"), "-s"])
    _make_dataset(aria, str(tmp_path), 6, w=640, h=480)          # 6 synthetic pairs
    exe = os.path.join(PKG, "euroc_frontend")
    t1, t2, tm = (str(tmp_path / n) for n in ("a.txt", "b.txt", "track.txt"))
    plain = subprocess.run([exe, str(tmp_path), "1000", "--pose", t1], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0, plain.stdout + plain.stderr
    run = subprocess.run([exe, str(tmp_path), "1000", "--pose", t2, "--track-map", tm], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert open(t1, "rb").read() == open(t2, "rb").read()
    n_frames = len(open(t1).read().splitlines())
    assert n_frames == 12
    line = [l.split() for l in run.stdout.splitlines() if l.startswith("track ")]
    assert len(line) == 1, run.stdout
    w = line[0]
    counts = dict(pnp=int(w[2]), fallback=int(w[4]), bootstrap=int(w[6]), held=int(w[8]))
    print(" ".join(w))
    assert sum(counts.values()) == n_frames - 1 and counts["bootstrap"] <= 1 and counts["pnp"] == 0
    pose_updates = int([l for l in run.stdout.splitlines() if l.startswith("pose updates")][0].split()[2])
    assert counts["bootstrap"] + counts["fallback"] == pose_updates          # every pose the stage accepted was taken
    rows = [l.split() for l in open(tm).read().splitlines()]
    assert len(rows) == n_frames and all(len(r) == 8 and all(np.isfinite(float(x)) for x in r) for r in rows)
    assert [float(x) for x in rows[0][1:]] == [0, 0, 0, 0, 0, 0, 1]          # the first frame is the map's frame
    bad = subprocess.run([exe, str(tmp_path), "1000", "--track-map", tm], capture_output=True, text=True, timeout=60)
    assert bad.returncode != 0 and "--pose" in bad.stderr
