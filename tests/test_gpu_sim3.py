"""Loop alignment on the MI355X (aria_sim3_*, kernels in aria_slam_amd/csrc/sim3_align.hip): hypotheses against the NumPy
restatement, the whole stage against it over the case table of tests/sim3_cases.py, batch == single and determinism, the
deferred errors, ground-truth accuracy, the join on the device and the device chain map -> join -> alignment, and the handle's
lifecycle. The reference project has no code for this stage: aria_slam_amd/sim3_ref.py is the definition."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sim3_cases as SC   # noqa: E402

pytestmark = pytest.mark.gpu

REC = 136                                                    # bytes of an aria_sim3_result
CORR = 64                                                    # bytes of an aria_sim3_corr
ARIA_E_INVALID, ARIA_E_NO_DEVICE = -1, -2

# The restatement's worst error against ground truth over SC.GT_CASES, measured on the CPU (tools/sim3_gap.py; pinned by
# tests/test_sim3_host.py): rotation 0.1034 deg, |t - t_true| / s 0.01361, |s / s_true - 1| 0.00588, mask precision 1.0.
# The device is allowed twice that.
GT_WORST = (0.1034, 0.01361, 0.00588, 1.0)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def est(aria):
    e = aria.HipSim3Aligner()
    yield e
    e.close()


def _aligner(aria, c, **kw):
    return aria.HipSim3Aligner(K=c.K, hypotheses=c.H, threshold_px=c.threshold_px, refine_iters=c.refine_iters,
                               fix_scale=c.fix_scale, min_scale=SC.MIN_SCALE, max_scale=SC.MAX_SCALE, seed=c.seed, **kw)


def _ulp32(x):
    return np.spacing(np.maximum(np.abs(np.asarray(x, np.float32)), np.float32(1e-30)))


@pytest.mark.parametrize("i", range(len(SC.SIM3_CASES)), ids=lambda i: SC.case_id(SC.SIM3_CASES[i]))
def test_hypotheses_against_the_restatement(aria, i):
    """aria_sim3_debug_hypotheses on every case of the table: the sample indices and the validity of every hypothesis are the
    restatement's; R, t and s agree to fp32 rounding of the restatement's values -- one fp32 unit in the last place of the
    largest entry of R (1), of t and of s, the most a last-bit difference of the fp64 closed form can move a rounding; each
    count equals the restatement's wherever no point of that hypothesis is in the band."""
    from aria_slam_amd import sim3_ref as N
    c = SC.SIM3_CASES[i]
    rep = SC.report(c)
    e = _aligner(aria, c)
    try:
        if c.nonfinite >= 0:
            with pytest.raises(aria._lib.AriaError) as err:
                e.debug_hypotheses(rep["corr"], c.pair_base)
            assert err.value.status == ARIA_E_INVALID and e.status() == 0
            return
        idx, R, t, s, cnt = e.debug_hypotheses(rep["corr"], c.pair_base)
    finally:
        e.close()
    ridx, rR, rt, rs, rcnt = rep["hyp"]
    assert idx.shape == (c.H, 3) and np.array_equal(idx, ridx)
    assert np.array_equal(cnt >= 0, rcnt >= 0)
    live = np.flatnonzero(rcnt >= 0)
    assert not R[rcnt < 0].any() and not t[rcnt < 0].any() and not s[rcnt < 0].any()
    if not len(live):
        return
    assert (np.abs(R[live] - rR[live]) <= _ulp32(1.0)).all()
    assert (np.abs(t[live] - rt[live]) <= _ulp32(np.abs(rt[live]).max(axis=1, keepdims=True))).all()
    assert (np.abs(s[live] - rs[live]) <= _ulp32(rs[live])).all()
    st = rep["staged"]
    thr2 = N.threshold2(c.threshold_px, c.K)
    for a in range(0, len(live), 256):
        sel = live[a:a + 256]
        near = (np.abs(N.error_ratio(rR[sel], rt[sel], rs[sel], st, thr2) - 1.0) < SC.BAND).sum(axis=1)
        assert (np.abs(cnt[sel] - rcnt[sel]) <= near).all()     # equal wherever no point of the hypothesis is in the band
    same = (R[live] == rR[live]).all(axis=1) & (t[live] == rt[live]).all(axis=1) & (s[live] == rs[live])
    print("case %d: %d of %d hypotheses valid, %d models bitwise equal" % (i, len(live), c.H, int(same.sum())))
    if c.n == 4096:                                        # the counts reach past the first LDS tile
        tail = {k: (v[SC.TILE:] if isinstance(v, np.ndarray) else v) for k, v in st.items()}
        beyond = N.inliers32(rR[live[:64]], rt[live[:64]], rs[live[:64]], tail, thr2).sum(axis=1)
        assert (beyond > 0).sum() >= 5


# ---- the whole stage against sim3_ref.estimate over the case table (tests/sim3_cases.py) -----------------------------------
# GAP, measured on the CPU with the committed restatement (tools/sim3_gap.py prints these tables): per exact-set case, the
# largest difference of R, t, s and rms_px between sim3_ref's fp64 run and its np.longdouble run.
SIM3_GAP = {    # case: (R, t, s, rms_px)
     2: (3.53e-16, 2.64e-15, 1.13e-16, 3.52e-14),    # s3-n3-H64
     3: (8.52e-16, 1.21e-14, 7.05e-14, 6.38e-14),    # s4-n4-H64
     4: (3.13e-16, 6.57e-16, 3.41e-15, 2.07e-14),    # s5-n7-H1024
     5: (5.58e-11, 1.07e-11, 2.54e-11, 4.54e-10),    # s6-n40-H320
     6: (4.85e-16, 1.04e-15, 4.07e-15, 1.47e-14),    # s7-n40-H64
     7: (6.23e-16, 1.28e-14, 4.47e-14, 4.32e-15),    # s8-n40-H1024
     8: (1.57e-14, 2.87e-14, 2.28e-16, 6.82e-14),    # s9-n150-H320
    10: (1.31e-16, 8.51e-16, 1.44e-15, 1.27e-15),    # s110-n600-H320
    11: (5.64e-16, 1.70e-15, 2.74e-15, 3.04e-15),    # s12-n600-H1024
    12: (1.30e-16, 2.18e-16, 2.02e-17, 2.80e-15),    # s13-n600-H64
    13: (4.31e-15, 5.93e-15, 1.12e-14, 2.13e-15),    # s14-n2047-H320
    14: (2.01e-13, 9.17e-14, 2.99e-13, 2.87e-13),    # s15-n2047-H64
    15: (4.69e-16, 8.57e-16, 1.24e-15, 1.20e-15),    # s160-n2048-H320
    16: (3.21e-16, 2.76e-16, 4.95e-16, 1.51e-15),    # s173-n2048-H64
    17: (2.13e-14, 1.23e-13, 3.78e-13, 1.30e-14),    # s180-n2049-H64
    18: (1.97e-15, 3.88e-15, 1.34e-14, 6.94e-15),    # s19-n2049-H320
    19: (8.66e-16, 3.53e-16, 1.65e-15, 2.78e-16),    # s223-n4096-H320
    20: (2.87e-16, 2.70e-16, 1.13e-15, 1.24e-15),    # s21-n300-H4096
    21: (1.56e-14, 2.98e-14, 1.77e-16, 2.65e-12),    # s22-n150-H320
    22: (3.96e-16, 1.05e-15, 0.00e+00, 1.04e-14),    # s23-n150-H320
    23: (1.09e-11, 3.66e-11, 0.00e+00, 2.84e-11),    # s240-n150-H320
    24: (4.56e-15, 2.62e-15, 1.55e-16, 1.27e-14),    # s25-n150-H320
    27: (2.68e-16, 2.84e-16, 7.73e-16, 3.36e-14),    # s28-n150-H1024
    28: (2.94e-15, 7.56e-15, 2.22e-14, 2.26e-13),    # s28-n150-H1024
    30: (3.55e-15, 8.55e-15, 1.79e-14, 2.39e-14),    # s30-n150-H320
}
SIM3_BATCH_GAP = {    # pair: (R, t, s, rms_px)
     0: (2.75e-16, 2.81e-16, 7.91e-16, 2.79e-15),    # s200-n300-H320
     2: (1.71e-14, 3.86e-14, 7.19e-14, 1.19e-14),    # s202-n2047-H320
     4: (2.14e-16, 7.13e-16, 2.14e-15, 3.76e-16),    # s204-n2048-H320
     5: (4.16e-14, 3.42e-13, 1.16e-15, 3.30e-12),    # s205-n3-H320
     6: (1.18e-13, 1.74e-13, 5.72e-13, 1.36e-13),    # s206-n2049-H320
     7: (5.01e-15, 7.58e-15, 1.67e-14, 7.96e-14),    # s207-n40-H320
     8: (2.58e-15, 6.43e-15, 2.02e-14, 4.34e-15),    # s208-n600-H320
    10: (4.46e-16, 2.28e-16, 1.10e-15, 2.29e-15),    # s210-n150-H320
}


def _compare(r, rep, gap, label):
    """One device result against the restatement's report of the case (tests/sim3_cases.py). Exact-set cases: every integer
    field and the mask equal, R, t, s and rms_px within 10 * GAP of the extended run. Other cases: the winner equal, the
    counts within the in-band points, the mask different only at those points."""
    c, ref, ext = rep["case"], rep["ref"], rep["ext"]
    assert r["n_corr"] == ref["n_corr"], label
    if rep["exact"]:
        for k in ("valid", "best_hypothesis", "iterations", "refined", "n_inliers"):
            assert r[k] == ref[k], (label, k, r[k], ref[k])
        assert r["mask"].tobytes() == ref["mask"].tobytes(), label
        if not ref["valid"]:
            assert np.array_equal(r["R"], np.eye(3)) and not r["t"].any() and r["s"] == 1.0 and r["rms_px"] == 0.0, label
            return
        d = SC.diff(r, ext)
        print("%s: R %.2e (allowed %.2e)  t %.2e (allowed %.2e)  s %.2e (allowed %.2e)  rms_px %.2e (allowed %.2e)" %
              (label, d[0], 10 * gap[0], d[1], 10 * gap[1], d[2], 10 * gap[2], d[3], 10 * gap[3]))
        assert all(d[k] <= 10 * gap[k] for k in range(4)), label
        return
    soft = rep["in_band"]
    assert r["valid"] == ref["valid"] == 1 and r["best_hypothesis"] == ref["best_hypothesis"], label
    assert abs(r["n_inliers"] - ref["n_inliers"]) <= soft, label
    assert not ((r["mask"] != ref["mask"]) & ~rep["soft"]).any(), label
    if ref["refit"] is not None and abs(ref["n_refit"] - ref["n_winner"]) > soft:
        assert r["refined"] == ref["refined"], label
    print("%s: not exact-set (%d in-band): n_inliers %d / %d, mask differs at %d" %
          (label, rep["in_band"], r["n_inliers"], ref["n_inliers"], int((r["mask"] != ref["mask"]).sum())))


@pytest.mark.parametrize("i", range(len(SC.SIM3_CASES)), ids=lambda i: SC.case_id(SC.SIM3_CASES[i]))
def test_whole_stage_equals_the_restatement(aria, i):
    """aria_sim3_estimate against sim3_ref.estimate on every case of the table: counts 0, 2, 3, 4, 7, mid sizes, around the
    2048-correspondence tile and 4096; H = 64, 320, 1024, 4096; seeds 0, 3 and one with the top bit set; pair ids 0, 5,
    1 000 000; true scales 0.25, 1, 4; outliers 0 to 0.5; both fix_scale values; no refinement; a planar cloud; a collinear
    cloud; all-equal correspondences; ties won by the first valid hypothesis; a true s beyond max_scale; landmarks behind a
    camera; a coordinate that is not finite. tests/test_sim3_host.py proves with the restatement alone that every case can
    be decided and what the table covers.

    Tolerance: measured, not chosen. The device is allowed 10 * GAP against the restatement's np.longdouble run, GAP being
    the fp64 run's own distance from it (SIM3_GAP above, tools/sim3_gap.py): the project's standing margin for another
    summation order. GAP is measured on the restatement, never on the device.

    GAP as measured (the case numbers index the table of tests/sim3_cases.py):
        case  n      H      R         t         s         rms_px
        2     3      64     3.53e-16  2.64e-15  1.13e-16  3.52e-14
        3     4      64     8.52e-16  1.21e-14  7.05e-14  6.38e-14
        4     7      1024   3.13e-16  6.57e-16  3.41e-15  2.07e-14
        5     40     320    5.58e-11  1.07e-11  2.54e-11  4.54e-10
        6     40     64     4.85e-16  1.04e-15  4.07e-15  1.47e-14
        7     40     1024   6.23e-16  1.28e-14  4.47e-14  4.32e-15
        8     150    320    1.57e-14  2.87e-14  2.28e-16  6.82e-14
        10    600    320    1.31e-16  8.51e-16  1.44e-15  1.27e-15
        11    600    1024   5.64e-16  1.70e-15  2.74e-15  3.04e-15
        12    600    64     1.30e-16  2.18e-16  2.02e-17  2.80e-15
        13    2047   320    4.31e-15  5.93e-15  1.12e-14  2.13e-15
        14    2047   64     2.01e-13  9.17e-14  2.99e-13  2.87e-13
        15    2048   320    4.69e-16  8.57e-16  1.24e-15  1.20e-15
        16    2048   64     3.21e-16  2.76e-16  4.95e-16  1.51e-15
        17    2049   64     2.13e-14  1.23e-13  3.78e-13  1.30e-14
        18    2049   320    1.97e-15  3.88e-15  1.34e-14  6.94e-15
        19    4096   320    8.66e-16  3.53e-16  1.65e-15  2.78e-16
        20    300    4096   2.87e-16  2.70e-16  1.13e-15  1.24e-15
        21    150    320    1.56e-14  2.98e-14  1.77e-16  2.65e-12
        22    150    320    3.96e-16  1.05e-15  0.00e+00  1.04e-14
        23    150    320    1.09e-11  3.66e-11  0.00e+00  2.84e-11
        24    150    320    4.56e-15  2.62e-15  1.55e-16  1.27e-14
        27    150    1024   2.68e-16  2.84e-16  7.73e-16  3.36e-14
        28    150    1024   2.94e-15  7.56e-15  2.22e-14  2.26e-13
        30    150    320    3.55e-15  8.55e-15  1.79e-14  2.39e-14
    Cases 0, 1, 25, 26, 29 and 31 (invalid) and 9, 32 (not exact-set) have no row: R, t, s and rms_px are not compared there.
    The s of cases 22 and 23 (fix_scale) is exactly 1 on both sides."""
    c = SC.SIM3_CASES[i]
    rep = SC.report(c)
    e = _aligner(aria, c)
    try:
        if c.nonfinite >= 0:                               # the host form reports the refusal; the record: test_deferred_errors
            with pytest.raises(aria._lib.AriaError) as err:
                e.estimate(rep["corr"], c.pair_base)
            assert err.value.status == ARIA_E_INVALID and e.status() == 0
            return
        r = e.estimate(rep["corr"], c.pair_base)
    finally:
        e.close()
    _compare(r, rep, SIM3_GAP.get(i), "case %d (%s)" % (i, SC.case_id(c)))


def _pack(torch, corrs, cap, dev, counts=None):
    """Device blocks for a list of correspondence arrays: pair p at p * cap (64 B each), and the counts."""
    B = len(corrs)
    cc = np.zeros((B, cap, CORR), np.uint8)
    nc = np.zeros(B, np.int32)
    for p, c in enumerate(corrs):
        cc[p, :len(c)] = np.ascontiguousarray(c).view(np.uint8).reshape(-1, CORR)
        nc[p] = len(c)
    if counts is not None:
        nc[:] = counts
    return torch.from_numpy(cc).to(dev), torch.from_numpy(nc).to(dev)


def _run_batch(est, bufs, cap, lo, hi, pair_base, out, mask):
    cc, nc = bufs
    est.estimate_batch_device(cc.data_ptr() + lo * cap * CORR, nc.data_ptr() + lo * 4, hi - lo, cap, out.data_ptr() + lo * REC,
                              mask.data_ptr() + lo * cap, pair_base)


def _launch(torch, e, corrs, cap, base, dev, splits=None, counts=None):
    """One launch (or the same pairs split into several calls) into fresh outputs: (status, records, masks)."""
    B = len(corrs)
    bufs = _pack(torch, corrs, cap, dev, counts)
    out = torch.zeros(B * REC, dtype=torch.uint8, device=dev)
    mask = torch.full((B * cap,), 7, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()                       # the handle's own stream is not ordered against torch's default stream
    splits = splits or (0, B)
    for a, b in zip(splits[:-1], splits[1:]):
        _run_batch(e, bufs, cap, a, b, base + a, out, mask)
    status = e.status()
    return status, out.cpu().numpy().tobytes(), mask.cpu().numpy().reshape(B, cap)


def test_batch_launch_equals_the_restatement_the_host_calls_a_split_and_a_second_run(aria, torch_cuda):
    """aria_sim3_estimate_batch_device, one launch over SC.SIM3_BATCH: 300, 0, 2047, 2, 2048, 3, 2049, 40, 600, 1 and 150
    correspondences side by side under one configuration, each pair against sim3_ref.estimate with its own pair id
    (tolerances: SIM3_BATCH_GAP), against the per-pair host call byte for byte, against the same launch split into two calls
    byte for byte, and against a second run byte for byte.

    GAP as measured (tools/sim3_gap.py prints it; by pair of the launch):
        pair  n      R         t         s         rms_px
        0     300    2.75e-16  2.81e-16  7.91e-16  2.79e-15
        2     2047   1.71e-14  3.86e-14  7.19e-14  1.19e-14
        4     2048   2.14e-16  7.13e-16  2.14e-15  3.76e-16
        5     3      4.16e-14  3.42e-13  1.16e-15  3.30e-12
        6     2049   1.18e-13  1.74e-13  5.72e-13  1.36e-13
        7     40     5.01e-15  7.58e-15  1.67e-14  7.96e-14
        8     600    2.58e-15  6.43e-15  2.02e-14  4.34e-15
        10    150    4.46e-16  2.28e-16  1.10e-15  2.29e-15
    """
    from aria_slam_amd.sim3 import _result_dict
    torch = torch_cuda
    dev = torch.device("cuda", 0)
    cases = SC.SIM3_BATCH
    cap = max(c.n for c in cases)
    corrs = [SC.report(c)["corr"] for c in cases]
    e = _aligner(aria, cases[0])
    try:
        status, out, mk = _launch(torch, e, corrs, cap, SC.BATCH_BASE, dev)
        assert status == 0
        rec = np.frombuffer(out, aria._lib.SIM3_RESULT_DTYPE)
        for p, c in enumerate(cases):
            assert not mk[p, c.n:].any(), p
            _compare(_result_dict(rec[p], mk[p, :c.n].copy()), SC.report(c), SIM3_BATCH_GAP.get(p), "pair %d (%s)" % (p, SC.case_id(c)))
            host = e.estimate(corrs[p], SC.BATCH_BASE + p)
            assert out[p * REC:(p + 1) * REC] == host["record"] and np.array_equal(mk[p, :c.n], host["mask"]), p
        again = _launch(torch, e, corrs, cap, SC.BATCH_BASE, dev)
        split = _launch(torch, e, corrs, cap, SC.BATCH_BASE, dev, splits=(0, 4, len(cases)))
        for other in (again, split):
            assert other[0] == 0 and other[1] == out and np.array_equal(other[2], mk)
        # a pair's place in a launch does not matter: alone in a launch of its own, under its own pair id
        for p in (8, 0):
            s1, o1, m1 = _launch(torch, e, [corrs[p]], cap, SC.BATCH_BASE + p, dev)
            assert s1 == 0 and o1 == out[p * REC:(p + 1) * REC] and np.array_equal(m1[0], mk[p])
    finally:
        e.close()


def test_deferred_errors_are_reported_once_and_leave_the_neighbours_untouched(aria, torch_cuda):
    """A count of corr_cap + 1 (and -1), and a pair with one coordinate that is not finite (NaN, +Inf in X1, X2 or a pixel),
    in the middle of the mixed launch: ARIA_E_INVALID once from check, the pair's record invalid with n_corr = 0 and a zero
    mask, every other pair's bytes those of the clean launch."""
    torch = torch_cuda
    dev = torch.device("cuda", 0)
    cases = SC.SIM3_BATCH
    cap = max(c.n for c in cases)
    corrs = [SC.report(c)["corr"] for c in cases]
    e = _aligner(aria, cases[0])
    try:
        status, clean, clean_mk = _launch(torch, e, corrs, cap, SC.BATCH_BASE, dev)
        assert status == 0

        def check_launch(got, victim):
            status, out, mk = got
            assert status == ARIA_E_INVALID and e.status() == 0                      # reported once
            for p in range(len(cases)):
                if p == victim:
                    r = np.frombuffer(out[p * REC:(p + 1) * REC], aria._lib.SIM3_RESULT_DTYPE)[0]
                    assert r["valid"] == 0 and r["n_corr"] == 0 and r["n_inliers"] == 0 and r["best_hypothesis"] == -1
                    assert r["s"] == 1.0 and np.array_equal(r["R"].reshape(3, 3), np.eye(3)) and not r["t"].any() and not mk[p].any()
                else:
                    assert out[p * REC:(p + 1) * REC] == clean[p * REC:(p + 1) * REC] and np.array_equal(mk[p], clean_mk[p]), p

        for victim, bad in ((4, cap + 1), (8, -1)):
            counts = [c.n for c in cases]
            counts[victim] = bad
            check_launch(_launch(torch, e, corrs, cap, SC.BATCH_BASE, dev, counts=counts), victim)
        for victim, field, row, fill in ((8, "X2", 77, np.nan), (0, "X1", 0, np.inf), (6, "u1", SC.TILE, np.nan), (10, "v2", 149, -np.inf)):
            dirty = [c.copy() for c in corrs]
            if field in ("X1", "X2"):
                dirty[victim][field][row, 1] = fill
            else:
                dirty[victim][field][row] = fill
            check_launch(_launch(torch, e, dirty, cap, SC.BATCH_BASE, dev), victim)
        # values that are finite but beyond fp32 never score and refuse nothing
        big = [c.copy() for c in corrs]
        big[8]["X2"][5:25, 2] = 1e300
        status, out, mk = _launch(torch, e, big, cap, SC.BATCH_BASE, dev)
        r = np.frombuffer(out[8 * REC:9 * REC], aria._lib.SIM3_RESULT_DTYPE)[0]
        assert status == 0 and r["valid"] == 1 and not mk[8, 5:25].any() and np.isfinite(np.frombuffer(out[8 * REC:8 * REC + 112], np.float64)).all()
        again = _launch(torch, e, corrs, cap, SC.BATCH_BASE, dev)
        assert again[0] == 0 and again[1] == clean and np.array_equal(again[2], clean_mk)      # the handle is sound
    finally:
        e.close()


def test_ground_truth(aria):
    """The device's similarity and mask against the scene's truth over SC.GT_CASES (0.5 px noise, 1 % depth noise, 0 to 50 %
    outliers, 40 to 4096 correspondences, true scales 0.25, 1 and 4). Bounds: twice the restatement's own worst error over
    the same cases, measured on the CPU -- rotation 0.1034 deg, |t - t_true| / s 0.01361, |s / s_true - 1| 0.00588, mask
    precision 1.0 (tools/sim3_gap.py; tests/test_sim3_host.py pins the four numbers)."""
    worst = [0.0, 0.0, 0.0, 1.0]
    for i in SC.GT_CASES:
        c = SC.SIM3_CASES[i]
        rep = SC.report(c)
        e = _aligner(aria, c)
        try:
            r = e.estimate(rep["corr"], c.pair_base)
        finally:
            e.close()
        assert r["valid"] == 1, i
        rot, tr, sc, prec = SC.truth_error(r, rep)
        worst = [max(worst[0], rot), max(worst[1], tr), max(worst[2], sc), min(worst[3], prec)]
        assert rot <= 2 * GT_WORST[0] and tr <= 2 * GT_WORST[1] and sc <= 2 * GT_WORST[2], (i, rot, tr, sc)
        assert prec >= 1.0 - 2 * (1.0 - GT_WORST[3]), (i, prec)
    print("device worst over %d cases: rotation %.4f deg, translation / s %.5f, relative scale %.5f, mask precision %.4f" %
          ((len(SC.GT_CASES),) + tuple(worst)))


def _project(X, R, t, K):
    fx, fy, cx, cy = K
    Xc = X @ np.asarray(R).T + t
    return np.stack([fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy], axis=1)


def test_device_chain_map_join_alignment(aria, est, torch_cuda):
    """A synthetic 3-D scene seen by four views. Views 0 and 1 are triangulated into the map as pair 11 at their true unit
    baseline; views 2 and 3, whose true baseline is 0.5, as pair 12 from a pose record of unit length, in view 2's frame: that
    part of the map is the scene at twice its size -- a drifted scale. Keyframe 1 is view 1 (view 2 of pair 11), keyframe 2 is
    view 2 (view 1 of pair 12). Their matches are joined with the map (aria_sim3_associate_batch_device) and aligned
    (aria_sim3_estimate_batch_device), all on one stream with no host step between.

    The join equals sim3_ref.associate on the fetched map byte for byte: a keypoint with two map points takes the one at the
    lowest arena position, a match with a point missing on either side yields nothing, match order is kept. Three pairs in
    one call: the first has its match list exactly full (n_matches = match_cap), the second an empty match list, the third
    an anchor the map does not hold. The alignment equals the host form on the fetched correspondences byte for byte, finds
    s = 2 and the relative pose within the ground-truth bounds, and an out-of-range match index is a deferred error of its
    pair alone."""
    from aria_slam_amd import _lib
    from aria_slam_amd import pose_ref as P
    from aria_slam_amd import sim3_ref as N
    torch = torch_cuda
    dev = torch.device("cuda", 0)
    K = P.EUROC_K
    rng = np.random.default_rng(77)
    n = 400
    u, v, z = rng.uniform(80, 670, n), rng.uniform(60, 420, n), rng.uniform(4, 12, n)
    X = np.stack([(u - K[2]) / K[0] * z, (v - K[3]) / K[1] * z, z], axis=1)
    Ra, ta = P.rot([0, 1, 0], 4), np.array([1.0, 0.0, 0.0])                   # view 1 from view 0: a unit baseline
    Rb, tb = P.rot([0.1, 1, 0], -6), np.array([-0.8, 0.1, 0.3])               # view 2 from view 0
    Rc, tc = P.rot([0, 1, 0.1], 3), np.array([0.5, 0.0, 0.0])                 # view 3 from view 2: half a unit
    R3, t3 = Rc @ Rb, Rc @ tb + tc
    views = [(np.eye(3), np.zeros(3)), (Ra, ta), (Rb, tb), (R3, t3)]
    perms = [np.arange(n)] + [rng.permutation(n) for _ in range(3)]          # point i is keypoint perm[i] of its view
    kps = []
    for (R, t), perm in zip(views, perms):
        k = np.zeros(n, _lib.KP_DTYPE)
        px = _project(X, R, t, K) + rng.normal(0, 0.3, (n, 2))
        k["x"][perm], k["y"][perm] = px[:, 0], px[:, 1]
        k["size"], k["response"] = 31.0, 1.0
        kps.append(k)
    # pair 11 maps points 0..299, pair 12 points 100..399: 100..299 are owned by both keyframes
    m01, m23 = np.zeros(300, _lib.MATCH_DTYPE), np.zeros(300, _lib.MATCH_DTYPE)
    m01["query_idx"], m01["train_idx"] = perms[0][:300], perms[1][:300]
    m23["query_idx"], m23["train_idx"] = perms[2][100:], perms[3][100:]
    # two map points on one keypoint of keyframe 1 (view 1) and of keyframe 2 (view 2): the other view's keypoint of the
    # neighbouring point lies half a pixel from its neighbour's, so both matches triangulate
    kps[0]["x"][151], kps[0]["y"][151] = kps[0]["x"][150] + 0.5, kps[0]["y"][150]
    m01["train_idx"][151] = perms[1][150]
    kps[3]["x"][perms[3][181]], kps[3]["y"][perms[3][181]] = kps[3]["x"][perms[3][180]] + 0.5, kps[3]["y"][perms[3][180]]
    m23["query_idx"][81] = perms[2][180]
    pose = np.zeros(2, _lib.POSE_RESULT_DTYPE)
    pose["R"][0], pose["t"][0] = Ra.ravel(), ta
    pose["R"][1], pose["t"][1] = Rc.ravel(), tc / np.linalg.norm(tc)          # unit length: the map's scale doubles
    pose["valid"], pose["n_inliers"], pose["n_pose_inliers"], pose["n_matches"] = 1, 300, 300, 300
    # the loop matches: keyframe 1 = view 1 (query), keyframe 2 = view 2 (train); 15 % hit another keypoint
    order = rng.permutation(n)
    loop = np.zeros(n, _lib.MATCH_DTYPE)
    loop["query_idx"], loop["train_idx"] = perms[1][order], perms[2][order]
    wrong = rng.permutation(n)[:60]
    loop["train_idx"][wrong] = perms[2][order[np.roll(wrong, 1)]]
    pose1 = np.concatenate([Ra, ta[:, None]], axis=1).ravel()                 # world (view 0's frame) to keyframe 1
    pose2 = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1).ravel()     # pair 12's points are in keyframe 2's frame
    B = 3
    work = torch.cuda.Stream(device=dev)
    mp = aria.HipMapper(stream=work.cuda_stream)
    al = aria.HipSim3Aligner(stream=work.cuda_stream)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)   # noqa: E731
    try:
        with torch.cuda.stream(work):
            d_kq, d_kt = up(np.concatenate([kps[0], kps[2]])), up(np.concatenate([kps[1], kps[3]]))
            d_m, d_nm, d_nk, d_pose = up(np.concatenate([m01, m23])), up(np.array([300, 300], np.int32)), up(np.array([n, n], np.int32)), up(pose)
            d_k1, d_k2 = up(np.concatenate([kps[1]] * B)), up(np.concatenate([kps[2]] * B))
            d_nB = up(np.full(B, n, np.int32))
            d_loop, d_nloop = up(np.concatenate([loop] * B)), up(np.array([n, 0, n], np.int32))
            d_a1, d_a2 = up(np.array([11, 11, 11], np.int32)), up(np.array([12, 12, 99], np.int32))
            d_p1, d_p2 = up(np.concatenate([pose1] * B)), up(np.concatenate([pose2] * B))
            d_corr = torch.zeros(B * n * CORR, dtype=torch.uint8, device=dev)
            d_ncorr = torch.full((B,), -7, dtype=torch.int32, device=dev)
            d_back = torch.full((B * n,), -7, dtype=torch.int32, device=dev)
            d_out = torch.zeros(B * REC, dtype=torch.uint8, device=dev)
            d_mask = torch.full((B * n,), 7, dtype=torch.uint8, device=dev)
        work.synchronize()
        mp.triangulate_batch_device(d_kq, d_nk, d_kt, d_nk, n, d_m, d_nm, 2, 300, d_pose=d_pose, query_is_first=True, pair_base=11)
        al.associate_batch_device(mp, d_a1, d_a2, 2, 1, d_p1, d_p2, d_k1, d_nB, d_k2, d_nB, n, d_loop, d_nloop, B, n, d_corr, d_ncorr, d_back)
        al.estimate_batch_device(d_corr, d_ncorr, B, n, d_out, d_mask, pair_base=40)   # straight from the join, no host copy
        mp.check()
        al.check()
        points = mp.read()
        ncorr = d_ncorr.cpu().numpy()
        corr = np.frombuffer(d_corr.cpu().numpy().tobytes(), _lib.SIM3_CORR_DTYPE).reshape(B, n)
        back = d_back.cpu().numpy().reshape(B, n)
        rec = d_out.cpu().numpy().tobytes()
        mask = d_mask.cpu().numpy().reshape(B, n)
    finally:
        al.close()
        mp.close()
    assert 500 <= len(points) <= 600 and set(points["pair"].tolist()) == {11, 12}
    assert (points["idx2"][points["pair"] == 11] == perms[1][150]).sum() == 2      # the duplicated keypoints are in the map twice
    assert (points["idx1"][points["pair"] == 12] == perms[2][180]).sum() == 2
    want_corr, want_back = N.associate(points, 11, 12, 2, 1, pose1, pose2, kps[1], kps[2], loop, kp_stride=n)
    assert ncorr.tolist() == [len(want_corr), 0, 0] and 120 <= ncorr[0] < 260
    assert corr[0, :ncorr[0]].tobytes() == want_corr.tobytes() and np.array_equal(back[0, :ncorr[0]], want_back)
    assert (back[0, :ncorr[0]][1:] > back[0, :ncorr[0]][:-1]).all()              # match order, stably compacted
    host = est.estimate(want_corr, 40)
    assert rec[:REC] == host["record"] and np.array_equal(mask[0, :ncorr[0]], host["mask"]) and not mask[0, ncorr[0]:].any()
    for p in (1, 2):
        r = np.frombuffer(rec[p * REC:(p + 1) * REC], _lib.SIM3_RESULT_DTYPE)[0]
        assert r["valid"] == 0 and r["n_corr"] == 0 and not mask[p].any()
    # the similarity: X2 = 2 (Rb Ra^T (X1 - ta) + tb)
    R_true = Rb @ Ra.T
    t_true = 2.0 * (tb - R_true @ ta)
    assert host["valid"] == 1 and host["n_inliers"] > 0.6 * ncorr[0]
    # bounds: twice the restatement's own error on the same correspondences (triangulated landmarks are noisier along their
    # rays than the table's scenes); and the drift is found: 0.3 px on baselines of 1 and 0.5 at depths 4 to 12 is a few
    # per cent of depth per landmark, far less over a hundred of them
    ref = N.estimate(want_corr, pair=40)
    err = lambda r: (N.rotation_error_deg(np.asarray(r["R"], np.float64), R_true),   # noqa: E731
                     float(np.linalg.norm(np.asarray(r["t"], np.float64) - t_true)) / 2.0, abs(float(r["s"]) / 2.0 - 1.0))
    assert ref["valid"] == 1 and all(d <= 2 * w + 1e-12 for d, w in zip(err(host), err(ref))), (err(host), err(ref))
    assert abs(host["s"] / 2.0 - 1.0) < 0.05
    print("chain: %d correspondences, %d inliers, s %.5f, rms %.3f px" % (ncorr[0], host["n_inliers"], host["s"], host["rms_px"]))
    # an out-of-range match index, and a count beyond match_cap, are deferred errors of their pairs alone
    bad = loop.copy()
    bad["train_idx"][17] = n
    mp = aria.HipMapper()
    al = aria.HipSim3Aligner()
    try:
        d_loop, d_nloop = up(np.concatenate([bad, loop, loop])), up(np.array([n, n, n + 1], np.int32))
        d_ncorr = torch.full((B,), -7, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        al.associate_batch_device(mp, d_a1, d_a2, 2, 1, d_p1, d_p2, d_k1, d_nB, d_k2, d_nB, n, d_loop, d_nloop, B, n, d_corr, d_ncorr)
        assert al.status() == ARIA_E_INVALID and al.status() == 0
        assert d_ncorr.cpu().numpy().tolist() == [0, 0, 0]                    # an empty map: nothing to join
    finally:
        al.close()
        mp.close()


# ---- the handle's lifecycle, in the manner of tests/test_gpu_handles.py ------------------------------------------------------
def test_create_rejects_a_bad_config_and_leaves_no_handle(aria, torch_cuda):
    L = aria.load_library()
    cfg = aria._lib.Sim3Config()
    L.aria_sim3_default_config(C.byref(cfg))
    assert cfg.struct_size == C.sizeof(cfg)
    h = C.c_void_p()
    cfg.struct_size += 4
    assert L.aria_sim3_create(C.byref(cfg), C.byref(h)) == ARIA_E_INVALID and not h.value
    cfg.struct_size -= 4
    cfg.device = torch_cuda.cuda.device_count()
    assert L.aria_sim3_create(C.byref(cfg), C.byref(h)) == ARIA_E_NO_DEVICE and not h.value
    assert ("device %d not present" % cfg.device) in L.aria_last_hip_error().decode()


def test_a_borrowed_stream_is_reported_and_survives_close(aria, torch_cuda):
    torch = torch_cuda
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(device=dev)
    h = aria.HipSim3Aligner(stream=s.cuda_stream)
    own = aria.HipSim3Aligner()
    try:
        assert h.stream == s.cuda_stream
        assert own.stream and own.stream != s.cuda_stream
        for x in (h, own):
            assert x.status() == 0
            x.check()
    finally:
        h.close()
        own.close()
    h.close()                                                     # a second close is a no-op
    with torch.cuda.stream(s):
        x = torch.arange(8, device=dev) * 2
    s.synchronize()
    assert int(x.sum()) == 56


def test_destroy_with_work_in_flight_and_a_grown_handle(aria, torch_cuda):
    """A launch is enqueued and the handle destroyed at once: destroy drains the stream, the outputs are complete and equal a
    fresh handle's. Then 40, 2049, 40 correspondences through one handle: the grown workspace computes what a fresh one does."""
    torch = torch_cuda
    dev = torch.device("cuda", 0)
    cases = SC.SIM3_BATCH
    cap = max(c.n for c in cases)
    corrs = [SC.report(c)["corr"] for c in cases]
    e = _aligner(aria, cases[0])
    status, want, want_mk = _launch(torch, e, corrs, cap, SC.BATCH_BASE, dev)
    e.close()
    assert status == 0
    bufs = _pack(torch, corrs, cap, dev)
    out = torch.zeros(len(cases) * REC, dtype=torch.uint8, device=dev)
    mask = torch.full((len(cases) * cap,), 7, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    e = _aligner(aria, cases[0])
    _run_batch(e, bufs, cap, 0, len(cases), SC.BATCH_BASE, out, mask)
    e.close()                                                     # no check, no synchronize in between
    assert out.cpu().numpy().tobytes() == want and np.array_equal(mask.cpu().numpy().reshape(len(cases), cap), want_mk)
    big = SC.report(SC.SIM3_CASES[18])["corr"]                     # 2049 correspondences
    fresh = {}
    for n in (40, 2049):
        f = aria.HipSim3Aligner(hypotheses=64)
        fresh[n] = f.estimate(big[:n], 2)
        f.close()
    g = aria.HipSim3Aligner(hypotheses=64)
    try:
        for n in (40, 2049, 40):
            r = g.estimate(big[:n], 2)
            assert r["record"] == fresh[n]["record"] and np.array_equal(r["mask"], fresh[n]["mask"]), n
    finally:
        g.close()
    assert fresh[2049]["valid"] == 1 and fresh[2049]["n_inliers"] > 1000
