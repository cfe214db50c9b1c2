"""Local bundle adjustment on the MI355X (aria_ba_*, kernel in aria_slam_amd/csrc/ba_schur.hip) against the NumPy restatement
(aria_slam_amd/ba_ref.py): the linearisation, the LM run at every iteration count of every case of tests/ba_cases.py, the
bits of what is fixed, invalid windows, determinism over batch position, batch split and scratch slots, the ground
truth of the generated scenes, and the track builder (aria_ba_window_from_chain_device) bit for bit against
ba_ref.window_from_chain on a chain triangulated by the map stage.

Tolerance of the LM comparison. The device takes its sums in another order than the restatement, so it is held to it by a
measured bound: ten times the case's CPU-measured gap at that iteration count (ba_cases.GAPS, from tools/ba_gap.py: the
restatement against its own full solve and against its own sums reversed), every difference scaled by max(1, |value|) as
there. The discrete fields are equal. tests/test_ba_host.py proves on the CPU that no decision of a case is near enough to
rho = 0, or to min_depth, for a summation order to flip it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ba_cases as BC   # noqa: E402

pytestmark = pytest.mark.gpu

ARIA_E_INVALID = -1
FIELDS = ("iterations_done", "trials", "stop_reason", "valid", "n_obs_used")


@pytest.fixture(scope="module")
def ba(aria):
    h = aria.HipBundleAdjuster(max_windows=4)
    yield h
    h.close()


@pytest.fixture(scope="module")
def ba_exact(aria):
    h = aria.HipBundleAdjuster(K=BC.EXACT_K, max_windows=2)
    yield h
    h.close()


def _same_bits_where_fixed(win, poses, points, used):
    """Fixed poses and points, and points with fewer than two used observations, keep their bits."""
    pf = win["pose_fixed"] != 0
    assert poses[pf].tobytes() == win["poses"][pf].tobytes()
    cnt = np.bincount(win["obs"]["point"][used != 0], minlength=len(win["points"]))
    held = (win["point_fixed"] != 0) | (cnt < 2)
    assert points[held].tobytes() == win["points"][held].tobytes()
    return int(pf.sum()), int(held.sum())


# ---- linearisation ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BC.LINEARIZE)
def test_linearisation_equals_the_restatement(ba, name):
    from aria_slam_amd import ba_ref as B
    win, _ = BC.scene(name)
    ref0 = B.linearize(win, 0.0)
    diag = [ref0["U"][i, k, k] for i in ref0["free_poses"] for k in range(6)] + \
           [ref0["V"][j, k, k] for j in ref0["free_points"] for k in range(3)]
    lam = 1e-5 * max(diag)
    ref = B.linearize(win, lam)
    got = ba.debug_linearize(win, lam)
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max()) if b.size else 0.0    # noqa: E731
    figs = dict(chi2=abs(got["chi2"] - ref["chi2"]) / ref["chi2"], S=rel(got["S"], ref["S"]), g=rel(got["g"], ref["g"]),
                V=rel(got["V"], ref["V"]), bp=rel(got["bp"], ref["bp"]))
    print("linearisation %s (%d free poses, %d used of %d observations):" % (name, len(ref["free_poses"]), ref["n_obs_used"],
                                                                            len(win["obs"])), figs)
    assert got["S"].shape == ref["S"].shape
    assert all(v <= 1e-9 for v in figs.values()), figs
    assert got["n_obs_used"] == ref["n_obs_used"]
    _p, _x, r = ba.optimize(win, 1)
    assert np.array_equal(r["used"], ref["used"])


# ---- LM against the restatement, every case with 1, 2, ..., K iterations ---------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in BC.CASES if c.name not in BC.EXEMPT])
def test_lm_equals_the_restatement_at_every_iteration_count(ba, name):
    from aria_slam_amd import ba_ref as B
    win, _ = BC.scene(name)
    c = BC.BY_NAME[name]
    worst = 0.0
    for k in range(1, c.K + 1):
        p, x, r = ba.optimize(win, k)
        pr, xr, rr = BC.reference_at(name, k)
        allow = 10 * BC.GAPS[name][k - 1]
        figs = dict(pose=BC.scaled(p, pr), point=BC.scaled(x, xr), lam=BC.scaled(r["lambda_"], rr["lambda_"]),
                    chi2=BC.scaled(r["chi2_final"], rr["chi2_final"]), rms=BC.scaled(r["rms_px"], rr["rms_px"]))
        share = {q: v / allow for q, v in figs.items()}
        worst = max(worst, max(share.values()))
        print("%s k=%d: chi2 %.6g -> %.6g rms %.4g px, %d trials; share of the allowance %s" %
              (name, k, r["chi2_initial"], r["chi2_final"], r["rms_px"], r["trials"],
               " ".join("%s %.3f" % kv for kv in share.items())))
        assert tuple(r[f] for f in FIELDS) == tuple(rr[f] for f in FIELDS), (k, r, rr)
        assert r["chi2_initial"] == pytest.approx(rr["chi2_initial"], rel=1e-12)
        assert all(np.isfinite(v) for v in (r["chi2_initial"], r["chi2_final"], r["lambda_"], r["rms_px"]))
        assert all(v <= allow for v in figs.values()), (k, figs, allow)
        assert np.array_equal(r["used"], BC.reference(name)[2]["used"])
        _same_bits_where_fixed(win, p, x, r["used"])
    print("%s: largest share of an allowance %.3f" % (name, worst))


def test_exact_case_is_exact(ba_exact):
    """chi2 = 0 and b = 0 without rounding: ten zero steps, rho == 0 rejected by rho > 0, and every figure equal."""
    win, _ = BC.scene("exact")
    pr, xr, rr = BC.reference("exact")
    assert BC.pattern(rr) == "r" * 10
    p, x, r = ba_exact.optimize(win, BC.BY_NAME["exact"].K)
    assert tuple(r[f] for f in FIELDS) == tuple(rr[f] for f in FIELDS) == (0, 10, 1, 1, len(win["obs"]))
    assert r["chi2_initial"] == r["chi2_final"] == r["rms_px"] == 0.0
    assert r["lambda_"] == rr["lambda_"] > 0
    assert np.array_equal(p, pr) and np.array_equal(x, xr) and np.array_equal(p, win["poses"]) and np.array_equal(x, win["points"])
    _same_bits_where_fixed(win, p, x, r["used"])


# ---- invalid windows ----------------------------------------------------------------------------------------------------------------
def test_invalid_windows_are_refused_and_leave_their_neighbours_alone(ba):
    good, _ = BC.scene("tiny")
    other, _ = BC.scene("motion_only")
    alone = [ba.optimize(w, 2) for w in (good, other)]
    bad = BC.invalid_windows()
    assert len(bad) >= 9
    for name, w in bad:
        P, X, R, status = ba.optimize_batch([good, w, other], 2, raise_on_error=False)
        assert status == ARIA_E_INVALID, name
        assert ba.status() == 0, name                       # reported once
        r = R[1]
        assert (r["valid"], r["stop_reason"], r["iterations_done"], r["trials"], r["n_obs_used"]) == (0, 2, 0, 0, 0), (name, r)
        assert r["chi2_initial"] == r["chi2_final"] == r["lambda_"] == r["rms_px"] == 0.0
        assert not r["used"].any() and not r["used_tail"].any()
        assert P[1].tobytes() == np.ascontiguousarray(w["poses"]).tobytes(), name          # NaN and all: bitwise
        assert X[1].tobytes() == np.ascontiguousarray(w["points"]).tobytes(), name
        for b, a in ((0, alone[0]), (2, alone[1])):
            assert P[b].tobytes() == a[0].tobytes() and X[b].tobytes() == a[1].tobytes(), name
            assert R[b]["record"] == a[2]["record"], name
    # the host form refuses the same windows, with the result record filled
    for name, w in bad:
        if "n_obs" in w:
            continue                                       # a count the host form cannot be handed
        p, x, r = ba.optimize(w, 2, raise_on_error=False)
        assert r["status"] == ARIA_E_INVALID and (r["valid"], r["stop_reason"]) == (0, 2), name
        assert p.tobytes() == w["poses"].tobytes() and x.tobytes() == w["points"].tobytes()


# ---- determinism ----------------------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_batch_position_split_or_slots(aria, ba):
    names = ["reject_later", "partial", "tiny", "huber"]
    wins = [BC.scene(n)[0] for n in names]
    target = wins[0]
    alone = ba.optimize(target, 4)
    key = lambda p, x, r: (p.tobytes(), x.tobytes(), r["record"], r["used"].tobytes())    # noqa: E731
    want = key(*alone)
    assert key(*ba.optimize(target, 4)) == want                              # a second run
    for order in ([0, 1, 2, 3], [1, 0, 2, 3], [1, 2, 3, 0]):                  # first, in the middle, last
        P, X, R, status = ba.optimize_batch([wins[i] for i in order], 4)
        b = order.index(0)
        assert status == 0 and key(P[b], X[b], R[b]) == want, order
    whole = ba.optimize_batch(wins + wins[:2], 4)                             # 6 windows on 4 slots: two launches
    halves = [ba.optimize_batch(wins[:3], 4), ba.optimize_batch(wins[3:] + wins[:2], 4)]
    got = [key(whole[0][b], whole[1][b], whole[2][b]) for b in range(6)]
    split = [key(h[0][b], h[1][b], h[2][b]) for h in halves for b in range(3)]
    assert got == split and got[0] == got[4] == want
    one = aria.HipBundleAdjuster(max_windows=1)
    try:
        P, X, R, status = one.optimize_batch(wins, 4)
        assert status == 0 and [key(P[b], X[b], R[b]) for b in range(4)] == got[:4]
    finally:
        one.close()


# ---- ground truth ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BC.GROUND_TRUTH)
def test_adjusted_windows_are_nearer_the_truth(ba, name):
    """The device may end at twice the restatement's final errors (ba_cases.GT, pinned by test_ba_host.py)."""
    from aria_slam_amd import ba_ref as B
    win, truth = BC.scene(name)
    p, x, r = ba.optimize(win, BC.BY_NAME[name].K)
    before, after = B.truth_errors(win["poses"], win["points"], truth, win), B.truth_errors(p, x, truth, win)
    (_b, ref_after) = BC.GT[name]
    print("%s: pose error %.4g -> %.4g, point error %.4g -> %.4g (restatement ends at %.4g, %.4g)" %
          (name, before[0], after[0], before[1], after[1], ref_after[0], ref_after[1]))
    assert r["valid"] == 1 and r["chi2_final"] < r["chi2_initial"]
    assert after[0] < before[0] and after[1] < before[1]
    assert after[0] <= 2 * ref_after[0] and after[1] <= 2 * ref_after[1]


# ---- the track builder ------------------------------------------------------------------------------------------------------------------
def test_track_builder_equals_the_restatement_and_its_window_optimises(aria, ba):
    import torch
    from aria_slam_amd import _lib, ba_ref as B
    dev = torch.device("cuda", 0)
    kps, matches, nm, ext, win0, truth = BC.generated_chain()
    frames, n = kps.shape
    P, cap = frames - 1, matches.shape[1]
    work = torch.cuda.Stream(device=dev)
    mp = aria.HipMapper(stream=work.cuda_stream)
    bb = aria.HipBundleAdjuster(stream=work.cuda_stream, max_windows=4)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)   # noqa: E731
    pcap, ocap = 4 * n, 4 * n * frames
    # windows: the whole chain; its middle two pairs; the whole chain with too few observation slots; a window that leaves the chain
    first, npairs = np.array([30, 31, 30, 32], np.int32), np.array([4, 2, 4, 3], np.int32)
    try:
        with torch.cuda.stream(work):
            d_k1, d_k2, d_m, d_nm = up(kps[:-1]), up(kps[1:]), up(matches), up(nm)
            d_n, d_ext = up(np.full(P, n, np.int32)), up(ext)
            d_first, d_np = up(first), up(npairs)
            d_X = torch.zeros(4 * pcap * 3, dtype=torch.float64, device=dev)
            d_obs = torch.zeros(4 * ocap * 16, dtype=torch.uint8, device=dev)
            d_src = torch.full((4 * pcap,), -7, dtype=torch.int32, device=dev)
            d_cnt = torch.full((2, 4), -7, dtype=torch.int32, device=dev)
        work.synchronize()
        mp.triangulate_batch_device(d_k1, d_n, d_k2, d_n, n, d_m, d_nm, P, cap, d_extrinsics=d_ext, query_is_first=True, pair_base=30)
        bb.window_from_chain_device(mp, d_first, d_np, 4, 30, P, d_k1, d_n, d_k2, d_n, n, d_m, d_nm, cap, pcap, ocap, d_X, d_obs, d_src,
                                    d_cnt[0], d_cnt[1])
        mp.check()
        assert bb.status() == ARIA_E_INVALID and bb.status() == 0          # window 3 leaves the chain; reported once
        arena = mp.read()
        cnt = d_cnt.cpu().numpy()
        X = d_X.cpu().numpy().reshape(4, pcap, 3)
        obs = np.frombuffer(d_obs.cpu().numpy().tobytes(), _lib.BA_OBS_DTYPE).reshape(4, ocap)
        src = d_src.cpu().numpy().reshape(4, pcap)
        assert len(arena) > 2 * n and set(arena["pair"]) == {30, 31, 32, 33}
        for b in (0, 1):
            q0 = first[b] - 30
            sl = slice(q0, q0 + npairs[b])
            want = B.window_from_chain(arena, int(first[b]), int(npairs[b]), kps[:-1][sl], np.full(P, n)[sl], kps[1:][sl],
                                       np.full(P, n)[sl], matches[sl], nm[sl], pcap, ocap)
            assert want["error"] == 0 and (cnt[0, b], cnt[1, b]) == (want["n_points"], want["n_obs"])
            assert X[b, :cnt[0, b]].tobytes() == want["points"].tobytes()
            assert obs[b, :cnt[1, b]].tobytes() == want["obs"].tobytes()
            assert np.array_equal(src[b, :cnt[0, b]], want["point_src"])
            per = np.bincount(want["obs"]["point"])
            print("window %d: %d points, %d observations, tracks of %d..%d views" % (b, want["n_points"], want["n_obs"], per.min(), per.max()))
            assert per.min() == 2 and per.max() == npairs[b] + 1
        assert cnt[:, 3].tolist() == [0, 0]
        # a capacity too small: ARIA_E_OUTPUT_TOO_SMALL and counts 0, the neighbours as before
        small = int(cnt[1, 0]) - 1
        d_cnt2 = torch.full((2, 2), -7, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        bb.window_from_chain_device(mp, d_first, d_np, 1, 30, P, d_k1, d_n, d_k2, d_n, n, d_m, d_nm, cap, pcap, small, d_X, d_obs, d_src,
                                    d_cnt2[0], d_cnt2[1])
        assert bb.status() == aria._lib.ARIA_E_OUTPUT_TOO_SMALL and d_cnt2.cpu().numpy()[:, 0].tolist() == [0, 0]
        # an index out of range in a match list refuses the windows that hold that pair
        bad = matches.copy()
        bad[3][5]["train_idx"] = n
        d_bad = up(bad)
        torch.cuda.synchronize()
        bb.window_from_chain_device(mp, d_first, d_np, 2, 30, P, d_k1, d_n, d_k2, d_n, n, d_bad, d_nm, cap, pcap, ocap, d_X, d_obs, d_src,
                                    d_cnt2[0], d_cnt2[1])
        assert bb.status() == ARIA_E_INVALID
        got = d_cnt2.cpu().numpy()
        assert got[:, 0].tolist() == [0, 0] and got[:, 1].tolist() == [cnt[0, 1], cnt[1, 1]]     # window 1 does not hold pair 33
    finally:
        bb.close()
        mp.close()
    # the whole chain's window optimises: the true poses perturbed, the first two fixed
    w = B.make_window(win0["poses"], win0["pose_fixed"], X[0, :cnt[0, 0]], np.zeros(cnt[0, 0], np.uint8), obs[0, :cnt[1, 0]])
    assert B.check_window(w)
    p, x, r = ba.optimize(w, 5)
    pr, xr, rr = B.optimize(w, 5)
    print("chain window: chi2 %.6g -> %.6g, rms %.4g px, %d iterations; restatement %.6g" %
          (r["chi2_initial"], r["chi2_final"], r["rms_px"], r["iterations_done"], rr["chi2_final"]))
    assert r["valid"] == 1 and r["chi2_final"] <= r["chi2_initial"] and r["iterations_done"] >= 1
    assert r["rms_px"] < 1.0 and r["chi2_final"] == pytest.approx(rr["chi2_final"], rel=1e-6)
