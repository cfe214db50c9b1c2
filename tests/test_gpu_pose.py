"""Two-view relative pose on the MI355X (aria_pose_*, kernels in aria_slam_amd/csrc/pose_ransac.hip): hypotheses against the
NumPy restatement, ground-truth accuracy, batch == single and determinism, edge cases, the device chain extract -> match ->
pose, and the C++ adapters."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "aria_slam_amd")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def est(aria):
    e = aria.HipPoseEstimator()
    yield e
    e.close()


def _motion(k):
    from aria_slam_amd import pose_ref as P
    R, t = [(np.eye(3), [0, 0, 1.0]), (np.eye(3), [1.0, 0, 0]), (P.rot([0.3, 1, 0.2], 5), [1, 0.3, 1.0]),
            (P.rot([0, 1, 0], 15), [0.5, 0, 1.0])][k % 4]
    t = np.asarray(t, np.float64)
    return R, t / np.linalg.norm(t)


def test_hypotheses_equal_the_reference(est):
    from aria_slam_amd import pose_ref as P
    R, t = _motion(3)
    kq, kt, m, _ = P.synth_two_view(7, 300, R, t, 0.3)
    idx, E, cnt = est.debug_hypotheses(kq, kt, m, pair_base=5)
    pts = P.normalise(kq, kt, m)
    ridx, rE, rcnt = P.hypotheses(pts, seed=0, pair=5, n_hyp=1024)
    assert np.array_equal(idx, ridx)                                     # the sample hash: exact
    both = (cnt >= 0) & (rcnt >= 0)
    assert both.sum() > 1000 and ((cnt >= 0) == (rcnt >= 0)).mean() > 0.99
    def canon(X):
        X = X / np.linalg.norm(X, axis=1, keepdims=True)
        s = np.sign(X[np.arange(len(X)), np.argmax(np.abs(X), axis=1)])
        return X * s[:, None]
    assert np.abs(canon(E[both].astype(np.float64)) - canon(rE[both])).max() < 1e-5
    thr2 = P.threshold2()
    err = P.sampson_error(rE[both], pts)
    near = (np.abs(err / thr2 - 1.0) < 1e-3).sum(axis=1)
    assert (np.abs(cnt[both] - rcnt[both]) <= near).all()


CASES = [(of, 1024, n) for of in (0.0, 0.2, 0.4) for n in (16, 200, 2000)] + [(0.5, 4096, n) for n in (200, 2000)]


@pytest.mark.parametrize("outliers,hyp,n", CASES)
def test_ground_truth(aria, outliers, hyp, n):
    """Synthetic scenes (2-20 m, sigma 0.5 px, unit baseline), the four motions of tests/test_pose_host.py in turn.
    n = 16 at 50 % outliers is left out: a clean 8-sample among 8 inliers of 16 is a 1 in 12870 draw."""
    from aria_slam_amd import pose_ref as P
    e = aria.HipPoseEstimator(hypotheses=hyp)
    try:
        for k in range(2):
            R, t = _motion(k + (n // 16))
            kq, kt, m, truth = P.synth_two_view(100 + k, n, R, t, outliers)
            r = e.estimate(kq, kt, m)
            assert r["valid"] == 1
            if n >= 200:
                assert P.rotation_error_deg(r["R"], R) < (0.5 if outliers <= 0.2 else 1.0)
                assert P.angle_deg(r["t"], t) < (3.0 if outliers <= 0.2 else 4.0)
            else:
                assert P.angle_deg(r["t"], t) < 15.0
            sel = r["mask"] == 1
            assert truth[sel].mean() >= (0.95 if n >= 200 else 0.85)     # n = 16: one outlier in the mask is 0.1
            # one refit from a noisy 8-point winner: recall is what the single refit reaches
            assert sel[truth].mean() >= (0.85 if outliers == 0.0 and n >= 200 else 0.5)
            assert r["n_pose_inliers"] == int(sel.sum()) and r["n_inliers"] >= r["n_pose_inliers"]
            assert np.isfinite(r["R"]).all() and np.isfinite(r["t"]).all()
    finally:
        e.close()


def _pack(torch, pairs, cap, dev):
    """Device blocks for pairs [(kq, kt, m)]: keypoints at p*cap (24 B each), matches at p*cap (12 B each)."""
    B = len(pairs)
    kq = np.zeros((B, cap, 24), np.uint8)
    kt = np.zeros((B, cap, 24), np.uint8)
    mm = np.zeros((B, cap, 12), np.uint8)
    nq = np.zeros(B, np.int32)
    nt = np.zeros(B, np.int32)
    nm = np.zeros(B, np.int32)
    for p, (a, b, m) in enumerate(pairs):
        kq[p, :len(a)] = a.view(np.uint8).reshape(-1, 24)
        kt[p, :len(b)] = b.view(np.uint8).reshape(-1, 24)
        mm[p, :len(m)] = m.view(np.uint8).reshape(-1, 12)
        nq[p], nt[p], nm[p] = len(a), len(b), len(m)
    t = lambda x: torch.from_numpy(x).to(dev)
    return t(kq), t(nq), t(kt), t(nt), t(mm), t(nm)


def _run_batch(torch, est, bufs, cap, lo, hi, pair_base, dev, out, mask):
    kq, nq, kt, nt, mm, nm = bufs
    est.estimate_batch_device(kq.data_ptr() + lo * cap * 24, nq.data_ptr() + lo * 4, kt.data_ptr() + lo * cap * 24,
                              nt.data_ptr() + lo * 4, cap, mm.data_ptr() + lo * cap * 12, nm.data_ptr() + lo * 4, hi - lo,
                              cap, out.data_ptr() + lo * 192, mask.data_ptr() + lo * cap, True, pair_base)


def _varied_pairs(n_pairs):
    from aria_slam_amd import pose_ref as P
    rng = np.random.default_rng(3)
    pairs = []
    for p in range(n_pairs):
        n = int(rng.choice([0, 5, 8, 12, 40, 150, 300, 600]))
        R, t = _motion(p)
        kq, kt, m, _ = P.synth_two_view(200 + p, max(n, 1), R, t, 0.3)
        pairs.append((kq[:n], kt[:n], m[:n]))
    return pairs


def test_batch_equals_single_and_is_deterministic(aria, est, torch_cuda):
    torch = torch_cuda
    dev = torch.device("cuda", 0)
    P_, cap, base = 64, 600, 100
    pairs = _varied_pairs(P_)
    bufs = _pack(torch, pairs, cap, dev)
    torch.cuda.synchronize()                       # the handle's own stream is not ordered against torch's default stream
    runs = []
    for split in ((0, 64), (0, 32, 64), (0, 64)):
        out = torch.zeros(P_ * 192, dtype=torch.uint8, device=dev)
        mask = torch.full((P_ * cap,), 7, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        for a, b in zip(split[:-1], split[1:]):
            _run_batch(torch, est, bufs, cap, a, b, base + a, dev, out, mask)
        est.check()
        runs.append((out.cpu().numpy().tobytes(), mask.cpu().numpy()))
    assert runs[0][0] == runs[2][0] and np.array_equal(runs[0][1], runs[2][1])     # run to run
    assert runs[0][0] == runs[1][0] and np.array_equal(runs[0][1], runs[1][1])     # split batch
    rec, mask = runs[0]
    n_valid = 0
    for p, (kq, kt, m) in enumerate(pairs):
        r = est.estimate(kq, kt, m, True, base + p)
        assert rec[p * 192:(p + 1) * 192] == r["record"], p
        assert np.array_equal(mask[p * cap:p * cap + len(m)], r["mask"]) and not mask[p * cap + len(m):(p + 1) * cap].any()
        n_valid += r["valid"]
    assert n_valid > P_ // 2


def test_edges(aria, est, torch_cuda):
    from aria_slam_amd import pose_ref as P
    R, t = _motion(0)
    kq, kt, m, _ = P.synth_two_view(9, 4096, R, t, 0.2)
    for n in (0, 7):
        r = est.estimate(kq, kt, m[:n])
        assert r["valid"] == 0 and not r["mask"].any() and np.array_equal(r["R"], np.eye(3)) and not r["t"].any()
        assert r["best_hypothesis"] == -1 and r["n_matches"] == n
    one = m[:50].copy()
    one["query_idx"] = 3
    one["train_idx"] = 3
    r = est.estimate(kq, kt, one)
    assert r["valid"] == 0 and not r["mask"].any()
    rec = np.frombuffer(r["record"], np.uint8)
    assert np.isfinite(np.frombuffer(rec[:168].tobytes(), np.float64)).all()
    r = est.estimate(kq, kt, m)                                             # n = match_cap = 4096
    assert r["valid"] == 1 and r["n_matches"] == 4096 and P.rotation_error_deg(r["R"], R) < 0.5
    # an out-of-range match index in the middle pair of three: reported, skipped, neighbours unaffected
    torch = torch_cuda
    dev = torch.device("cuda", 0)
    pairs = []
    for k in range(3):
        a, b, mk, _ = P.synth_two_view(30 + k, 200, *_motion(k), 0.2)
        pairs.append((a, b, mk))
    bad = pairs[1][2].copy()
    bad["train_idx"][17] = 200
    pairs[1] = (pairs[1][0], pairs[1][1], bad)
    cap = 200
    bufs = _pack(torch, pairs, cap, dev)
    out = torch.zeros(3 * 192, dtype=torch.uint8, device=dev)
    mask = torch.full((3 * cap,), 7, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    _run_batch(torch, est, bufs, cap, 0, 3, 0, dev, out, mask)
    assert est.status() == aria._lib.ARIA_OK - 1                            # ARIA_E_INVALID
    assert est.status() == aria._lib.ARIA_OK                                # reported once
    o = out.cpu().numpy().tobytes()
    mh = mask.cpu().numpy()
    for p in (0, 2):
        want = est.estimate(*pairs[p], True, p)
        assert o[p * 192:(p + 1) * 192] == want["record"] and np.array_equal(mh[p * cap:(p + 1) * cap], want["mask"])
    rec1 = np.frombuffer(o[192:384], aria._lib.POSE_RESULT_DTYPE)[0]
    assert rec1["valid"] == 0 and rec1["n_matches"] == 0 and not mh[cap:2 * cap].any()
    with pytest.raises(aria.AriaError):
        est.estimate(*pairs[1])                                              # the host form rejects it up front


def test_device_chain_extract_match_pose(aria, est, torch_cuda):
    """synth_sequence -> batch extract -> batch match (pair p: query f = p + 1, train f = p) -> batch pose, all on one
    stream, equals aria_pose_estimate on the fetched keypoints and matches. The synthetic pairs are a 2-D shift of a flat
    scene (degenerate for E): agreement and finiteness are checked, not accuracy."""
    torch = torch_cuda
    dev = torch.device("cuda", 0)
    W, H, NF = 640, 480, 2000
    seq = aria.synth_sequence(41, 3, W, H)
    B = len(seq)
    images = torch.from_numpy(seq).to(dev)
    work = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    e = aria.OrbHipExtractor(max_features=NF, stream=work.cuda_stream, max_width=W, max_height=H, max_batch=B)
    mt = aria.HipMatcher(stream=work.cuda_stream)
    pe = aria.HipPoseEstimator(stream=work.cuda_stream)
    try:
        cap = e.kp_capacity()
        with torch.cuda.stream(work):
            kps = torch.zeros((B, cap, 24), dtype=torch.uint8, device=dev)
            desc = torch.zeros((B, cap, 32), dtype=torch.uint8, device=dev)
            counts = torch.zeros((B,), dtype=torch.int32, device=dev)
            matches = torch.zeros((B, cap, 12), dtype=torch.uint8, device=dev)
            nm = torch.zeros((B,), dtype=torch.int32, device=dev)
            out = torch.zeros((B - 1) * 192, dtype=torch.uint8, device=dev)
            mask = torch.zeros((B - 1) * cap, dtype=torch.uint8, device=dev)
        work.synchronize()
        e.extract_batch_device(images, B, W, H, kps, desc, counts, cap)
        mt.match_batch_device(desc.data_ptr() + cap * 32, counts.data_ptr() + 4, desc, counts, B - 1, cap * 32, 0.75, matches,
                              nm, cap)
        pe.estimate_batch_device(kps.data_ptr() + cap * 24, counts.data_ptr() + 4, kps, counts, cap, matches, nm, B - 1, cap,
                                 out, mask, query_is_first=False, pair_base=0)
        e.check()
        mt.sync()
        pe.check()
        c = counts.cpu().numpy()
        k = kps.cpu().numpy()
        mh = matches.cpu().numpy()
        nmh = nm.cpu().numpy()
        o = out.cpu().numpy().tobytes()
        mk = mask.cpu().numpy()
        from aria_slam_amd._lib import KP_DTYPE, MATCH_DTYPE, POSE_RESULT_DTYPE
        assert (nmh[:B - 1] >= 8).all()
        for p in range(B - 1):
            kq = k[p + 1, :c[p + 1]].copy().view(KP_DTYPE).reshape(-1)
            kt = k[p, :c[p]].copy().view(KP_DTYPE).reshape(-1)
            m = mh[p, :nmh[p]].copy().view(MATCH_DTYPE).reshape(-1)
            want = est.estimate(kq, kt, m, False, p)
            assert o[p * 192:(p + 1) * 192] == want["record"], p
            assert np.array_equal(mk[p * cap:p * cap + nmh[p]], want["mask"])
            rec = np.frombuffer(o[p * 192:(p + 1) * 192], POSE_RESULT_DTYPE)[0]
            assert np.isfinite(rec["R"]).all() and np.isfinite(rec["t"]).all() and np.isfinite(rec["E"]).all()
    finally:
        pe.close()
        mt.close()
        e.close()


def test_cpp_pose_selftest(aria):
    subprocess.check_call(["make", "-C", os.path.join(PKG, "host"), "-s"])
    src = os.path.join(ROOT, "tests", "cpp", "pose_selftest.cpp")
    exe = os.path.join(ROOT, "build", "pose_selftest")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "host", "include"),
                           src, "-o", exe, "-L" + PKG, "-laria_hip_adapters", "-laria_orb_hip", "-lz", "-Wl,-rpath," + PKG])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "DONE" in out.stdout, out.stdout + out.stderr
    kv = {l.split()[0]: l.split()[1:] for l in out.stdout.splitlines() if l.strip()}
    assert kv["estimate"][0] == "1" and float(kv["estimate"][1]) < 0.5 and int(kv["estimate"][2]) > 100
    assert kv["verifier_reject"] == ["0"]                      # min_inliers above what the pair has: no loop
    assert kv["verifier_accept"][0] == "1" and kv["verifier_accept"][1] == kv["verifier_accept"][2]   # matches cut to inliers
    assert float(kv["verifier_accept"][3]) < 0.5               # relative_pose rotation = the scene's
    assert kv["frontend"][0] == "1" and kv["frontend"][1] == "1" and kv["frontend"][2] == "0"   # pose on frame 1, none on frame 0, off by default
