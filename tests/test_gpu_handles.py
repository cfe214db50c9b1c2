"""What every stage handle (aria_slam_amd._lib.STAGES) shares, on the MI355X: create-time rejection, the borrowed stream,
what the entry points answer to a null handle, the grow-only staging and workspace of the three match-list stages, and the
deferred input error. Every comparison is byte for byte against a fresh handle: a handle that has grown, or has reported an
error, computes what a new one computes."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STAGES = ["pose", "fund", "map", "graph", "fuse", "eval", "det", "stereo", "rect", "dense", "tsdf", "nav", "alert", "pnp", "ba", "ray",
          "icp", "mesh", "proj", "bow", "sim3"]
MATCH_STAGES = ["pose", "fund", "map"]
ARIA_E_INVALID, ARIA_E_NO_DEVICE = -1, -2
HYP = 64
SIZES = (40, 2049, 40)            # 2049 crosses the 2048-point LDS tile of the scoring kernels
BATCH_N = (200, 40, 0, 150, 200)  # matches per pair of the batch form; the first launch takes two pairs, the second all five
CAP = 200
W, H = 64, 48                     # the map stage's gray image


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def _config(aria, prefix):
    L = aria._lib
    return dict(pose=L.PoseConfig, fund=L.FundConfig, map=L.MapConfig, graph=L.GraphConfig, fuse=L.FuseConfig,
                eval=L.EvalConfig, det=L.DetConfig, stereo=L.StereoConfig, rect=L.RectConfig, dense=L.DenseConfig,
                tsdf=L.TsdfConfig, nav=L.NavConfig, alert=L.AlertConfig, pnp=L.PnpConfig, ba=L.BaConfig, ray=L.RayConfig,
                icp=L.IcpConfig, mesh=L.MeshConfig, proj=L.ProjConfig, bow=L.BowConfig, sim3=L.Sim3Config)[prefix]()


VOL = (16, 16, 16)                # the smallest volumes of whole 8^3 bricks with more than one brick per axis
SMALL = dict(pose=dict(hypotheses=HYP), fund=dict(hypotheses=HYP), pnp=dict(hypotheses=HYP), sim3=dict(hypotheses=HYP),
             rect=dict(src_size=(W, H)), dense=dict(max_size=(W, H)), alert=dict(width=W, height=H), ba=dict(max_windows=4),
             tsdf=dict(dims=VOL), ray=dict(dims=VOL), mesh=dict(dims=VOL), nav=dict(dims=VOL, max_goals=4),
             bow=dict(words=64, rows=64, capacity=16))


def _make(aria, prefix, **kw):
    """A handle of the stage at the smallest size it accepts where its create allocates by size (SMALL); every default
    config is creatable as it stands, rect's included (aria_rect_default_config fills in a camera)."""
    cls = dict(pose=aria.HipPoseEstimator, fund=aria.HipFundamentalEstimator, map=aria.HipMapper, graph=aria.HipPoseGraphOptimizer,
               fuse=aria.HipSensorFusion, eval=aria.HipTrajectoryEvaluator, det=aria.HipObjectDetector, stereo=aria.HipStereoMatcher,
               rect=aria.HipRectifier, dense=aria.HipDenseStereo, tsdf=aria.HipTsdfVolume, nav=aria.HipPathPlanner,
               alert=aria.HipObstacleAlerter, pnp=aria.HipPnPEstimator, ba=aria.HipBundleAdjuster, ray=aria.HipVolumeRenderer,
               icp=aria.HipDenseTracker, mesh=aria.HipVolumeMesher, proj=aria.HipProjectionMatcher, bow=aria.HipBowIndex,
               sim3=aria.HipSim3Aligner)[prefix]
    return cls(**SMALL.get(prefix, {}), **kw)


@pytest.mark.parametrize("prefix", STAGES)
def test_create_rejects_a_bad_config_and_leaves_no_handle(aria, torch_cuda, prefix):
    L = aria.load_library()
    create = getattr(L, "aria_%s_create" % prefix)
    cfg = _config(aria, prefix)
    getattr(L, "aria_%s_default_config" % prefix)(C.byref(cfg))
    assert cfg.struct_size == C.sizeof(cfg)
    h = C.c_void_p()
    cfg.struct_size += 4
    assert create(C.byref(cfg), C.byref(h)) == ARIA_E_INVALID and not h.value
    cfg.struct_size -= 4
    cfg.device = torch_cuda.cuda.device_count()
    assert create(C.byref(cfg), C.byref(h)) == ARIA_E_NO_DEVICE and not h.value
    assert ("device %d not present" % cfg.device) in L.aria_last_hip_error().decode()


@pytest.mark.parametrize("prefix", STAGES)
def test_a_borrowed_stream_is_reported_and_survives_close(aria, torch_cuda, prefix):
    torch = torch_cuda
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(device=dev)
    h = _make(aria, prefix, stream=s.cuda_stream)
    own = _make(aria, prefix)
    try:
        assert h.stream == s.cuda_stream
        assert own.stream and own.stream != s.cuda_stream
        for x in (h, own):
            assert x.status() == ((0, 0, 0) if prefix == "det" else 0)
            x.check()
    finally:
        h.close()
        own.close()
    h.close()                                                     # a second close is a no-op
    with torch.cuda.stream(s):
        x = torch.arange(8, device=dev) * 2
    s.synchronize()
    assert int(x.sum()) == 56


@pytest.mark.parametrize("prefix", STAGES)
def test_a_null_handle_is_refused_by_check_and_ignored_by_destroy_and_stream(aria, prefix):
    L = aria.load_library()
    fn = lambda name: getattr(L, "aria_%s_%s" % (prefix, name))   # noqa: E731
    assert fn("destroy")(None) is None
    assert fn("stream")(None) is None
    assert (fn("check")(None, None, None) if prefix == "det" else fn("check")(None)) == ARIA_E_INVALID


# ---- the three match-list stages: inputs, and one way to run each form ------------------------------------------------------
def _extrinsics():
    from aria_slam_amd import map_ref as M
    R1 = M.rot([0.1, 1, 0.2], 3)
    R2 = M.rot([0.2, 1, 0.1], -5) @ R1
    return M.extrinsics(R1, [0.3, -0.1, 0.2]), M.extrinsics(R2, [-1.5, 0.2, 0.3])


def _scene(prefix, seed, n):
    """(kp_query, kp_train, matches) with n matches; match i joins keypoint i of both views, so every prefix is a scene."""
    from aria_slam_amd import fund_ref as F, map_ref as M, pose_ref as P
    R, t = P.rot([0.3, 1, 0.2], 5), np.array([1, 0.3, 1.0]) / np.linalg.norm([1, 0.3, 1.0])
    if prefix == "pose":
        return P.synth_two_view(seed, n, R, t, 0.2)[:3]
    if prefix == "fund":
        return F.synth_two_view(seed, n, R, t, 0.2)[:3]
    return M.synth_scene(seed, n, *_extrinsics(), outlier_frac=0.2, depth=(1.0, 30.0))[:3]


@pytest.fixture(scope="module")
def inputs():
    """Per stage: the single-pair scene of max(SIZES) matches and the five pairs of the batch form. Read-only."""
    out = {}
    for prefix in MATCH_STAGES:
        kq, kt, m = _scene(prefix, 11, max(SIZES))
        pairs = []
        for p, n in enumerate(BATCH_N):
            a, b, mm = _scene(prefix, 20 + p, CAP)
            pairs.append((a[:n], b[:n], mm[:n]))
        out[prefix] = dict(single=(kq, kt, m), pairs=pairs)
    return out


def _image():
    return ((np.arange(W * H) * 7) % 256).astype(np.uint8).reshape(H, W)


def _single(prefix, h, scene, n):
    """The blocking host form on n matches: everything it returns, as bytes."""
    kq, kt, m = (x[:n] for x in scene)
    if prefix == "map":
        h.clear()
        added = h.triangulate(kq, kt, m, *_extrinsics(), image=_image(), pair_id=2)
        return added, h.read().tobytes()
    r = h.estimate(kq, kt, m, True, 2)
    return r["record"], r["mask"].tobytes()


def _pack(aria, torch, pairs, dev):
    B = len(pairs)
    kq, kt = np.zeros((B, CAP), aria.KP_DTYPE), np.zeros((B, CAP), aria.KP_DTYPE)
    mm = np.zeros((B, CAP), aria.MATCH_DTYPE)
    cnt = np.zeros((3, B), np.int32)
    for p, (a, b, m) in enumerate(pairs):
        kq[p, :len(a)], kt[p, :len(b)], mm[p, :len(m)] = a, b, m
        cnt[:, p] = len(a), len(b), len(m)
    ext = np.tile(np.concatenate([np.asarray(e, np.float64).reshape(-1)[:12] for e in _extrinsics()]), (B, 1))
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).to(dev)   # noqa: E731
    return dict(kq=t(kq), kt=t(kt), mm=t(mm), nq=t(cnt[0]), nt=t(cnt[1]), nm=t(cnt[2]), ext=t(ext))


def _batch(prefix, h, torch, b, n_pairs, dev):
    """The device batch form over the first n_pairs pairs of b into fresh outputs; returns them as bytes after check()."""
    B = len(BATCH_N)
    args = (b["kq"], b["nq"], b["kt"], b["nt"], CAP, b["mm"], b["nm"], n_pairs, CAP)
    if prefix == "map":
        h.clear()
        outs = [torch.full((B,), -1, dtype=torch.int32, device=dev)]
        torch.cuda.synchronize()
        h.triangulate_batch_device(*args, d_extrinsics=b["ext"], d_added=outs[0], pair_base=3)
    else:
        rec = 192 if prefix == "pose" else 96
        outs = [torch.zeros(B * rec, dtype=torch.uint8, device=dev), torch.full((B * CAP,), 7, dtype=torch.uint8, device=dev)]
        if prefix == "fund":
            outs += [torch.full((B * CAP * 12,), 9, dtype=torch.uint8, device=dev),
                     torch.full((B,), -5, dtype=torch.int32, device=dev)]
        torch.cuda.synchronize()                                  # the handle's stream is not ordered against torch's
        h.estimate_batch_device(*args, *outs, True, 3)
    status = h.status()
    got = [o.cpu().numpy().tobytes() for o in outs]
    if prefix == "map":
        got.append(h.read().tobytes())
    return status, got


@pytest.fixture(scope="module")
def fresh(aria, torch_cuda, inputs):
    """What a fresh handle returns for every input of the tests below, computed once: fresh[prefix]["single"][n] and
    fresh[prefix]["batch"]."""
    dev = torch_cuda.device("cuda", 0)
    out = {}
    for prefix in MATCH_STAGES:
        single = {}
        for n in sorted(set(SIZES)):
            h = _make(aria, prefix)
            single[n] = _single(prefix, h, inputs[prefix]["single"], n)
            h.close()
        h = _make(aria, prefix)
        status, batch = _batch(prefix, h, torch_cuda, _pack(aria, torch_cuda, inputs[prefix]["pairs"], dev), len(BATCH_N), dev)
        h.close()
        assert status == 0
        out[prefix] = dict(single=single, batch=batch)
    return out


@pytest.mark.parametrize("prefix", MATCH_STAGES)
def test_a_grown_handle_computes_what_a_fresh_one_does(aria, torch_cuda, inputs, fresh, prefix):
    """40, 2049, 40 matches through the blocking form of one handle: the second call grows every staging and workspace
    buffer, the third runs in the grown ones. Then the batch form on two pairs and on five."""
    dev = torch_cuda.device("cuda", 0)
    h = _make(aria, prefix)
    try:
        for n in SIZES:
            assert _single(prefix, h, inputs[prefix]["single"], n) == fresh[prefix]["single"][n], n
        b = _pack(aria, torch_cuda, inputs[prefix]["pairs"], dev)
        assert _batch(prefix, h, torch_cuda, b, 2, dev)[0] == 0
        assert _batch(prefix, h, torch_cuda, b, len(BATCH_N), dev) == (0, fresh[prefix]["batch"])
    finally:
        h.close()
    if prefix != "map":                                           # the inputs are not degenerate
        rec = np.frombuffer(fresh[prefix]["single"][2049][0], aria._lib.POSE_RESULT_DTYPE if prefix == "pose"
                            else aria._lib.FUND_RESULT_DTYPE)[0]
        assert rec["valid"] == 1 and rec["n_matches"] == 2049 and rec["n_inliers"] > 1000
    else:
        assert fresh[prefix]["single"][2049][0] > 1000 and fresh[prefix]["single"][40][0] > 20


@pytest.mark.parametrize("prefix", MATCH_STAGES)
def test_a_deferred_input_error_is_reported_once_and_leaves_the_handle_sound(aria, torch_cuda, inputs, fresh, prefix):
    dev = torch_cuda.device("cuda", 0)
    pairs = inputs[prefix]["pairs"]
    bad = pairs[0][2].copy()
    bad["train_idx"][17] = CAP                                     # one past the pair's last train keypoint
    h = _make(aria, prefix)
    try:
        status, _ = _batch(prefix, h, torch_cuda, _pack(aria, torch_cuda, [(pairs[0][0], pairs[0][1], bad)] + pairs[1:], dev),
                           1, dev)
        assert status == ARIA_E_INVALID
        assert h.status() == 0                                    # reported once
        assert _batch(prefix, h, torch_cuda, _pack(aria, torch_cuda, pairs, dev), len(BATCH_N), dev) == (0, fresh[prefix]["batch"])
    finally:
        h.close()


def test_stereo_scale_reports_a_bad_match_index_once_and_stays_sound(aria, torch_cuda):
    """The same for the stereo stage's batch form that takes a match list (aria_stereo_scale_batch_device): three poses
    (R = I, t = x) over 40 matched keypoints whose second view lies 0.5 further along t."""
    from aria_slam_amd import stereo_ref as R
    from aria_slam_amd._lib import MATCH_DTYPE, POSE_RESULT_DTYPE, STEREO_SCALE_DTYPE
    torch = torch_cuda
    dev = torch.device("cuda", 0)
    B, n = 3, 40
    rng = np.random.default_rng(1)
    first, second = R.unmatched_obs(n), R.unmatched_obs(n)
    first["X"], first["Y"], first["depth"] = rng.uniform(-2, 2, n), rng.uniform(-1, 1, n), rng.uniform(3, 8, n)
    second["X"], second["Y"], second["depth"] = first["X"] + np.float32(0.5), first["Y"], first["depth"]
    first["right_idx"] = second["right_idx"] = np.arange(n)
    pose = np.zeros(B, POSE_RESULT_DTYPE)
    pose["R"], pose["t"], pose["valid"], pose["n_pose_inliers"] = np.eye(3).reshape(-1), [1.0, 0.0, 0.0], 1, n
    m = np.zeros((B, n), MATCH_DTYPE)
    m["query_idx"] = m["train_idx"] = np.arange(n)
    bad = m.copy()
    bad[1, 3]["train_idx"] = n
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).to(dev)   # noqa: E731
    d_pose, d_first, d_second = t(pose), t(np.stack([first] * B)), t(np.stack([second] * B))
    d_cnt = t(np.full(B, n, np.int32))

    def run(h, matches):
        out = torch.full((B * 16,), 3, dtype=torch.uint8, device=dev)
        d_m = t(matches)
        torch.cuda.synchronize()
        h.scale_batch_device(d_pose, None, d_m, d_cnt, n, d_first, d_cnt, d_second, d_cnt, n, B, out)   # view 1 = query
        return h.status(), out.cpu().numpy().view(STEREO_SCALE_DTYPE).copy()

    fresh_h = aria.HipStereoMatcher()
    h = aria.HipStereoMatcher()
    try:
        status, want = run(fresh_h, m)
        assert status == 0 and (want["valid"] == 1).all() and (want["n_used"] == n).all()
        assert np.abs(want["scale"] - 0.5).max() < 1e-6
        status, got = run(h, bad)
        assert status == ARIA_E_INVALID and h.status() == 0        # reported once
        assert got[1]["valid"] == 0 and got[0].tobytes() == want[0].tobytes() and got[2].tobytes() == want[2].tobytes()
        assert run(h, m)[0] == 0 and run(h, m)[1].tobytes() == want.tobytes()
    finally:
        h.close()
        fresh_h.close()
