"""Guided matching on the MI355X (aria_proj_*, kernels in aria_slam_amd/csrc/proj_search.hip) against its definition, the NumPy
restatement aria_slam_amd/proj_ref.py: every byte of the aria_proj_obs records, the correspondences, the pairs and the counts is
equal, and on the case table (tests/proj_cases.py) equal to the answers written down from the construction as well. A
difference in a float field is a contraction or ordering bug, never a tolerance."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import proj_cases as PC   # noqa: E402

GUARD = 256                                   # bytes of 0x5A before and after every output
INVALID = -1                                  # ARIA_E_INVALID


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def work(torch_cuda):
    torch = torch_cuda
    s = torch.cuda.Stream(device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    return s


def _dev(torch, work, a):
    with torch.cuda.stream(work):
        t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")
    work.synchronize()
    return t


def _guarded(torch, work, nbytes):
    with torch.cuda.stream(work):
        t = torch.full((nbytes + 2 * GUARD,), 0x5A, dtype=torch.uint8, device="cuda:0")
    work.synchronize()
    return t


def _body(t, dtype):
    raw = t.cpu().numpy()
    assert (raw[:GUARD] == 0x5A).all() and (raw[-GUARD:] == 0x5A).all(), "a guard byte around an output was written"
    return raw[GUARD:-GUARD].copy().view(dtype)


def _search(torch, work, pm, poses, kps, descs, ns, kp_stride, width, height, landmarks, ranges, land_cap):
    """aria_proj_search_batch_device on host arrays -> (obs (F, land_cap), corr (F, land_cap), pairs (F, land_cap), ncorr (F,),
    status). Every output lies between guard bytes and starts as 0x5A."""
    from aria_slam_amd._lib import PNP_CORR_DTYPE, PROJ_OBS_DTYPE, PROJ_PAIR_DTYPE
    F = len(poses)
    d_pose = _dev(torch, work, np.asarray(poses, np.float64))
    d_kp, d_desc = _dev(torch, work, np.stack(kps)), _dev(torch, work, np.stack(descs))
    d_n, d_range = _dev(torch, work, np.asarray(ns, np.int32)), _dev(torch, work, np.asarray(ranges, np.int32))
    d_land = _dev(torch, work, landmarks)
    d_obs, d_corr = _guarded(torch, work, F * land_cap * 24), _guarded(torch, work, F * land_cap * 32)
    d_pairs, d_ncorr = _guarded(torch, work, F * land_cap * 8), _guarded(torch, work, F * 4)
    pm.search_batch_device(d_pose, d_kp, d_desc, d_n, kp_stride, width, height, d_land, len(landmarks), d_range, land_cap, F,
                           d_obs[GUARD:], d_corr[GUARD:], d_pairs[GUARD:], d_ncorr[GUARD:])
    status = pm.status()
    return (_body(d_obs, PROJ_OBS_DTYPE).reshape(F, land_cap), _body(d_corr, PNP_CORR_DTYPE).reshape(F, land_cap),
            _body(d_pairs, PROJ_PAIR_DTYPE).reshape(F, land_cap), _body(d_ncorr, np.int32), status)


def _assert_frame(tag, obs, corr, pairs, ncorr, want_obs, want_corr, want_pairs):
    for name in obs.dtype.names:
        bad = np.flatnonzero(obs[name].view(np.int32) != want_obs[name].view(np.int32))
        if len(bad):
            print("%s: field %s differs at %s: got %s want %s" % (tag, name, bad[:8], obs[name][bad[:8]], want_obs[name][bad[:8]]))
    assert obs.tobytes() == want_obs.tobytes(), tag
    assert ncorr == len(want_corr), (tag, ncorr, len(want_corr))
    assert corr[:ncorr].tobytes() == want_corr.tobytes() and pairs[:ncorr].tobytes() == want_pairs.tobytes(), tag
    assert (corr[ncorr:].view(np.uint8) == 0x5A).all() and (pairs[ncorr:].view(np.uint8) == 0x5A).all(), tag   # nothing beyond the count


@pytest.fixture(scope="module")
def table():
    """The case table with the restatement of every frame, computed once; the restatement equals the written-down answers
    (tests/test_proj_host.py holds it to them too)."""
    from aria_slam_amd import proj_ref as R
    t = PC.table()
    arrays = [PC.frame_arrays(f) for f in t["frames"]]
    want = []
    for f, (kp, desc) in zip(t["frames"], arrays):
        obs, corr, pairs, _ = R.search_frame_ref(f["pose"], kp, desc, f["n"], t["kp_stride"], t["landmarks"], f["first"], f["count"],
                                                 t["land_cap"], t["cfg"], t["width"], t["height"])
        known = PC.expected(f, t["landmarks"])
        assert obs.tobytes() == known[0].tobytes() and corr.tobytes() == known[1].tobytes() and pairs.tobytes() == known[2].tobytes()
        want.append((obs, corr, pairs))
    return dict(t, arrays=arrays, want=want)


def _run_table(aria, torch, work, table, order):
    pm = aria.HipProjectionMatcher(K=table["cfg"]["K"], stream=work.cuda_stream)
    try:
        fr = [table["frames"][i] for i in order]
        out = _search(torch, work, pm, [f["pose"] for f in fr], [table["arrays"][i][0] for i in order],
                      [table["arrays"][i][1] for i in order], [f["n"] for f in fr], table["kp_stride"], table["width"], table["height"],
                      table["landmarks"], [(f["first"], f["count"]) for f in fr], table["land_cap"])
        again = pm.status()
    finally:
        pm.close()
    return out, again


def _check_table(table, order, out):
    obs, corr, pairs, ncorr, _ = out
    for j, i in enumerate(order):
        _assert_frame(table["frames"][i]["name"], obs[j], corr[j], pairs[j], ncorr[j], *table["want"][i])
    assert np.isfinite(obs["u"]).all() and np.isfinite(obs["v"]).all()


def test_case_table_as_one_batch(aria, torch_cuda, work, table):
    order = list(range(len(table["frames"])))
    out, again = _run_table(aria, torch_cuda, work, table, order)
    assert out[4] == INVALID and again == 0                                   # the eight invalid frames: reported once
    _check_table(table, order, out)
    assert out[3].sum() > 300


def test_case_table_split_one_and_rest(aria, torch_cuda, work, table):
    F = len(table["frames"])
    first, _ = _run_table(aria, torch_cuda, work, table, [0])
    assert first[4] == 0                                                      # frame 0 is valid: no error of its own
    _check_table(table, [0], first)
    rest, _ = _run_table(aria, torch_cuda, work, table, list(range(1, F)))
    assert rest[4] == INVALID
    _check_table(table, list(range(1, F)), rest)


def test_case_table_in_reversed_batch_order(aria, torch_cuda, work, table):
    order = list(range(len(table["frames"])))[::-1]
    out, _ = _run_table(aria, torch_cuda, work, table, order)
    _check_table(table, order, out)


def test_run_to_run_repeat_has_equal_bytes(aria, torch_cuda, work, table):
    order = list(range(len(table["frames"])))
    a, _ = _run_table(aria, torch_cuda, work, table, order)
    b, _ = _run_table(aria, torch_cuda, work, table, order)
    for x, y in zip(a[:4], b[:4]):
        assert x.tobytes() == y.tobytes()


def test_real_descriptors_under_a_known_motion(aria, torch_cuda, work):
    """Two 320 x 240 / 500-feature frames from the device extractor. Landmarks are frame A's keypoints back-projected at a depth
    pattern; they are searched in frame A itself and in frame B of the pair under a small known motion, as one batch sharing
    the range."""
    from aria_slam_amd import proj_ref as R
    from aria_slam_amd._lib import KP_DTYPE, PROJ_LANDMARK_DTYPE
    torch = torch_cuda
    a, b = aria.synth_frame_pair(1, 320, 240)
    e = aria.OrbHipExtractor(max_features=500, max_width=320, max_height=240)
    fa, fb = e.extract(a), e.extract(b)
    e.close()
    ka, kb = fa["keypoints"].view(KP_DTYPE).reshape(-1), fb["keypoints"].view(KP_DTYPE).reshape(-1)
    da, db = fa["descriptors"].reshape(-1, 32), fb["descriptors"].reshape(-1, 32)
    assert len(ka) > 256 and len(kb) > 256
    K = R.EXACT_K
    z = 2.0 + (np.arange(len(ka)) % 5)
    lm = np.zeros(len(ka) + 2, PROJ_LANDMARK_DTYPE)
    n = len(ka)
    lm["X"][:n, 0], lm["X"][:n, 1], lm["X"][:n, 2] = (ka["x"].astype(np.float64) - K[2]) / K[0] * z, (ka["y"].astype(np.float64) - K[3]) / K[1] * z, z
    lm["desc"][:n], lm["octave"][:n], lm["source"][:n] = da, ka["octave"], np.arange(n)
    lm["octave"][n:] = -1
    ang = np.deg2rad(0.4)
    pose = np.array([np.cos(ang), 0, np.sin(ang), 0.01, 0, 1, 0, -0.005, -np.sin(ang), 0, np.cos(ang), 0.002])
    stride = max(len(ka), len(kb)) + 3
    land_cap = len(lm) + 5
    kps, descs = [], []
    for k, d in ((ka, da), (kb, db)):
        kk, dd = np.zeros(stride, KP_DTYPE), np.full((stride, 32), 0xA5, np.uint8)
        kk[:len(k)], dd[:len(k)] = k, d
        kk["x"][len(k):], kk["y"][len(k):] = 160, 120                         # beyond the count: nobody may read them
        kps.append(kk)
        descs.append(dd)
    cfg = dict(K=K)
    want = [R.search_frame_ref(pose, kps[f], descs[f], [len(ka), len(kb)][f], stride, lm, 0, len(lm), land_cap, cfg, 320, 240) for f in range(2)]
    pm = aria.HipProjectionMatcher(K=K, stream=work.cuda_stream)
    try:
        obs, corr, pairs, ncorr, status = _search(torch, work, pm, [pose, pose], kps, descs, [len(ka), len(kb)], stride, 320, 240, lm,
                                                  [(0, len(lm)), (0, len(lm))], land_cap)
    finally:
        pm.close()
    assert status == 0
    for f in range(2):
        _assert_frame("frame %d" % f, obs[f], corr[f], pairs[f], ncorr[f], *want[f][:3])
    print("real descriptors: %d landmarks, %d matched in frame A, %d in frame B" % (n, ncorr[0], ncorr[1]))
    won = obs[0]["flags"] & 8 != 0
    assert (obs[0]["hamming"][won] == 0).sum() > 0.5 * won.sum() and ncorr[0] > n // 4   # in A itself the true keypoint is in the window


def test_large_frame_of_4000_keypoints_and_5000_landmarks(aria, torch_cuda, work):
    """1408 x 1408 coordinates: 44 x 44 cells, twenty chunks of landmarks, windows of every octave; descriptors drawn from a pool
    of 20 so that ties, ratio rejections and lost claims are common."""
    from aria_slam_amd import proj_ref as R
    from aria_slam_amd._lib import KP_DTYPE, PROJ_LANDMARK_DTYPE
    rng = np.random.default_rng(31)
    NK, NL, S = 4000, 5000, 1408
    pool = R.random_descriptors(rng, 20)
    kp = np.zeros(NK, KP_DTYPE)
    kp["x"], kp["y"] = rng.uniform(-2, S + 2, NK).astype(np.float32), rng.uniform(-2, S + 2, NK).astype(np.float32)
    kp["octave"] = rng.integers(0, 8, NK)
    desc = pool[rng.integers(0, 20, NK)].copy()
    noise = rng.integers(0, 256, (NK, 32), dtype=np.uint8) & rng.integers(0, 256, (NK, 32), dtype=np.uint8) & rng.integers(0, 256, (NK, 32), dtype=np.uint8)
    desc ^= noise * (rng.random((NK, 1)) < 0.7)                               # 30 % exact copies of a pool entry
    K = (700.0, 700.0, 704.0, 704.0)
    lm = np.zeros(NL, PROJ_LANDMARK_DTYPE)
    z = rng.uniform(0.05, 9.0, NL)
    u, v = rng.uniform(-30, S + 30, NL), rng.uniform(-30, S + 30, NL)
    lm["X"] = np.stack([(u - K[2]) / K[0] * z, (v - K[3]) / K[1] * z, z], axis=1)
    lm["desc"] = pool[rng.integers(0, 20, NL)]
    lm["octave"] = rng.integers(-1, 9, NL)
    pose = np.array([1, 0, 0, 0.01, 0, 1, 0, 0.02, 0, 0, 1, 0.05], np.float64)
    cfg = dict(K=K)
    want = R.search_frame_ref(pose, kp, desc, NK, NK, lm, 0, NL, NL, cfg, S, S)
    pm = aria.HipProjectionMatcher(K=K, stream=work.cuda_stream)
    try:
        obs, corr, pairs, ncorr, status = _search(torch_cuda, work, pm, [pose], [kp], [desc], [NK], NK, S, S, lm, [(0, NL)], NL)
    finally:
        pm.close()
    assert status == 0
    _assert_frame("large", obs[0], corr[0], pairs[0], ncorr[0], *want[:3])
    flags = set(obs[0]["flags"].tolist())
    print("large frame: %d matched, flags seen %s" % (ncorr[0], sorted(flags)))
    assert {0, 1, 3, 7, 15} <= flags and ncorr[0] > 100


def _scene_views(rng, n):
    from aria_slam_amd import pose_ref as P
    K = P.EUROC_K
    u, v, z = rng.uniform(60, 690, n), rng.uniform(40, 440, n), rng.uniform(3, 12, n)
    X = np.stack([(u - K[2]) / K[0] * z, (v - K[3]) / K[1] * z, z], axis=1)
    return K, X, P


def test_join_from_a_device_built_map(aria, torch_cuda, work):
    """Two pairs triangulated into a HipMapper (pair ids 11 and 12), joined on the device with the keypoints and descriptors
    of their second views (slots 0 and 1) and held to landmarks_from_map_ref on the fetched arena; then the same with a slot
    count of 1, which puts pair 12 out of range: dead landmarks and ARIA_E_INVALID, once."""
    from aria_slam_amd import _lib
    from aria_slam_amd import proj_ref as R
    torch = torch_cuda
    rng = np.random.default_rng(77)
    n = 200
    K, X, P = _scene_views(rng, n)
    R2, t2 = P.rot([0, 1, 0], 4), np.array([1.0, 0.0, 0.0])
    proj = lambda Rm, t: (lambda Xc: np.stack([K[0] * Xc[:, 0] / Xc[:, 2] + K[2], K[1] * Xc[:, 1] / Xc[:, 2] + K[3]], axis=1))(X @ Rm.T + t)   # noqa: E731
    px1, px2 = proj(np.eye(3), np.zeros(3)), proj(R2, t2)
    stride = n + 8
    kp = np.zeros((2, 2, stride), _lib.KP_DTYPE)                              # [pair][view]
    perm = [rng.permutation(n), rng.permutation(n)]
    for p in range(2):
        kp[p, 0]["x"][:n], kp[p, 0]["y"][:n] = px1[:, 0], px1[:, 1]
        kp[p, 1]["x"][perm[p]], kp[p, 1]["y"][perm[p]] = px2[:, 0], px2[:, 1]
        kp[p, 1]["octave"][:n] = rng.integers(0, 8, n)
    desc = R.random_descriptors(rng, 2 * stride).reshape(2, stride, 32)       # of the second views
    counts = np.array([n, n - 20], np.int32)                                  # slot 1 says 180: idx2 >= 180 is out of range
    mp = aria.HipMapper(K=K, stream=work.cuda_stream)
    pm = aria.HipProjectionMatcher(K=K, stream=work.cuda_stream)
    try:
        for p in range(2):
            m = np.zeros(150, _lib.MATCH_DTYPE)
            m["query_idx"], m["train_idx"] = np.arange(150), perm[p][:150]
            mp.triangulate(kp[p, 0][:n], kp[p, 1][:n], m, np.hstack([np.eye(3), np.zeros((3, 1))]), np.hstack([R2, t2[:, None]]), pair_id=11 + p)
        size = mp.size()
        arena = mp.read()
        assert size > 200 and set(arena["pair"].tolist()) == {11, 12}
        d_kp, d_desc, d_n = _dev(torch, work, kp[:, 1]), _dev(torch, work, desc), _dev(torch, work, counts)
        for first, max_count, n_slots in ((0, size + 7, 2), (13, 100, 2), (0, size, 1), (size + 5, 4, 2)):
            d_land, d_nl = _guarded(torch, work, max(max_count, 1) * 64), _guarded(torch, work, 4)
            pm.landmarks_from_map_device(mp, first, max_count, 11, 2, d_kp, d_desc, d_n, stride, n_slots, d_land[GUARD:], d_nl[GUARD:])
            status, again = pm.status(), pm.status()
            want, cnt, invalid = R.landmarks_from_map_ref(arena, size, first, max_count, 11, 2, kp[:, 1], desc, counts, stride, n_slots)
            got = _body(d_land, _lib.PROJ_LANDMARK_DTYPE)[:max_count]
            assert _body(d_nl, np.int32)[0] == cnt and got.tobytes() == want.tobytes(), (first, max_count, n_slots)
            assert status == (INVALID if invalid else 0) and again == 0
            if n_slots == 1:
                assert invalid and (got["octave"][arena["pair"][:cnt] == 12] == -1).all()
        assert (want["octave"] == -1).all()                                   # the last range starts beyond the map: all dead
    finally:
        pm.close()
        mp.close()


def test_chain_search_then_pnp_returns_the_known_pose(aria, torch_cuda, work):
    """The exact scene seen from t = (0.125, -0.0625, 0): every landmark at depth 4 moves by (+8, -4) px and at depth 8 by
    (+4, -2) px, exactly. Searched from the predicted pose [I|0] (the true keypoint is inside the 15 px window), the
    correspondences go to aria_pnp_estimate_batch_device with corr_cap = land_cap on the same stream. The pixels are exact in
    fp32 and the points in fp64, so the refined pose has zero residual; the bound of 1e-6 map units and degrees is what fp64
    Gauss-Newton leaves of it, with three orders to spare."""
    from aria_slam_amd import _lib
    from aria_slam_amd import proj_ref as R
    torch = torch_cuda
    rng = np.random.default_rng(4)
    n = 150
    u, v = rng.permutation(280)[:n] + 20, rng.integers(20, 220, n)            # distinct columns
    z = np.where(np.arange(n) % 2 == 0, 4.0, 8.0)
    D = R.random_descriptors(rng, n)
    lm = np.concatenate([R.make_landmark(int(u[i]), int(v[i]), D[i], z=z[i]) for i in range(n)])
    order = rng.permutation(n)
    kp = np.concatenate([R.make_keypoint(u[i] + 32.0 / z[i], v[i] - 16.0 / z[i]) for i in order])
    desc = D[order]
    t_true = np.array([0.125, -0.0625, 0.0])
    want = R.search_frame_ref(R.IDENTITY_POSE, kp, desc, n, n, lm, 0, n, n, dict(K=R.EXACT_K), 320, 240)
    pm = aria.HipProjectionMatcher(K=R.EXACT_K, stream=work.cuda_stream)
    pe = aria.HipPnPEstimator(K=R.EXACT_K, stream=work.cuda_stream)
    try:
        d_pose, d_kp, d_desc = _dev(torch, work, R.IDENTITY_POSE), _dev(torch, work, kp), _dev(torch, work, desc)
        d_n, d_range, d_land = _dev(torch, work, np.array([n], np.int32)), _dev(torch, work, np.array([0, n], np.int32)), _dev(torch, work, lm)
        d_obs, d_corr, d_pairs = _guarded(torch, work, n * 24), _guarded(torch, work, n * 32), _guarded(torch, work, n * 8)
        d_ncorr, d_out, d_mask = _guarded(torch, work, 4), _guarded(torch, work, 128), _guarded(torch, work, n)
        pm.search_batch_device(d_pose, d_kp, d_desc, d_n, n, 320, 240, d_land, n, d_range, n, 1, d_obs[GUARD:], d_corr[GUARD:],
                               d_pairs[GUARD:], d_ncorr[GUARD:])
        pe.estimate_batch_device(d_corr[GUARD:], d_ncorr[GUARD:], 1, n, d_out[GUARD:], d_mask[GUARD:])
        assert pm.status() == 0 and pe.status() == 0
        ncorr = _body(d_ncorr, np.int32)[0]
        _assert_frame("chain", _body(d_obs, _lib.PROJ_OBS_DTYPE), _body(d_corr, _lib.PNP_CORR_DTYPE), _body(d_pairs, _lib.PROJ_PAIR_DTYPE),
                      ncorr, *want[:3])
        res = _body(d_out, _lib.PNP_RESULT_DTYPE)[0]
        mask = _body(d_mask, np.uint8)
    finally:
        pe.close()
        pm.close()
    assert ncorr == n                                                         # random descriptors: nothing competes
    Rm = res["R"].reshape(3, 3)
    rot_deg = np.degrees(np.arccos(np.clip((np.trace(Rm) - 1) / 2, -1, 1)))
    print("chain: n_inliers %d of %d, |t - t*| %.3g, rotation %.3g deg, rms %.3g px" % (res["n_inliers"], ncorr, np.linalg.norm(res["t"] - t_true),
                                                                                    rot_deg, res["rms_px"]))
    assert res["valid"] == 1 and res["n_inliers"] == n and mask.all()
    assert np.linalg.norm(res["t"] - t_true) <= 1e-6 and rot_deg <= 1e-6


def test_handle_lifecycle_on_a_borrowed_and_an_owned_stream(aria, torch_cuda, work, table):
    """The blocking host form on a handle that owns its stream and on one that borrows the test's; the borrowed stream outlives
    the handle."""
    torch = torch_cuda
    f = [f for f in table["frames"] if f["name"] == "repeated texture"][0]
    lm = table["landmarks"][f["first"]:f["first"] + f["count"]]
    want_obs = f["exp"]
    for stream in (None, work.cuda_stream):
        pm = aria.HipProjectionMatcher(K=table["cfg"]["K"], stream=stream)
        assert (pm.stream == work.cuda_stream) == (stream is not None) and pm.stream
        for _ in range(2):                                                    # the staging is reused
            obs, corr, pairs = pm.search(f["pose"], f["kp"], f["desc"], lm, table["width"], table["height"])
            assert obs.tobytes() == want_obs.tobytes() and len(corr) == len(pairs) == 12
            assert sorted(pairs["landmark"].tolist()) == list(range(12))      # the host form searches its own array: first = 0
        obs, corr, pairs = pm.search(f["pose"], f["kp"][:0], f["desc"][:0], lm, table["width"], table["height"])
        assert len(corr) == 0 and (obs["flags"] == 1).all()
        bad = f["pose"].copy()
        bad[3] = np.nan
        with pytest.raises(aria.AriaError):
            pm.search(bad, f["kp"], f["desc"], lm, table["width"], table["height"])
        assert pm.status() == 0
        pm.close()
        pm.close()                                                            # idempotent
    with torch.cuda.stream(work):
        t = torch.ones(16, device="cuda:0").sum()
    work.synchronize()
    assert float(t) == 16.0
