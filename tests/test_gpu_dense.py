"""Dense stereo on the MI355X (aria_dense_*, kernels in aria_slam_amd/csrc/dense_stereo.hip) against its definition, the NumPy
restatement aria_slam_amd/dense_ref.py: every disparity, every depth and every sampled record is BITWISE equal. The stage is
integer arithmetic up to the disparity map, so a difference is a bug, never a tolerance."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_cases as DC   # noqa: E402


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
        t = torch.from_numpy(np.array(a).view(np.uint8).reshape(-1)).to("cuda:0")       # a copy: the shared cases are read-only
    work.synchronize()
    return t


def _full(torch, work, nbytes, value):
    with torch.cuda.stream(work):
        t = torch.full((max(nbytes, 1),), value, dtype=torch.uint8, device="cuda:0")
    work.synchronize()
    return t


def _handle(aria, work, size, **kw):
    return aria.HipDenseStereo(K=DC.K, baseline=DC.BASELINE, max_size=size, stream=work.cuda_stream, **kw)


def _run(torch, work, h, pairs, padded=False, depth=True):
    """The batch form over `pairs` -> (d16 (n, H, W), depth (n, H, W) or None, True when no padding element changed)."""
    n, (H, W) = len(pairs), pairs[0][0].shape
    ip, istr, dp, dstr, zp, zstr = (DC.IMG_PITCH, DC.IMG_STRIDE, DC.DISP_PITCH, DC.DISP_STRIDE, DC.DEPTH_PITCH,
                                    DC.DEPTH_STRIDE) if padded else (W, W * H, W, W * H, W, W * H)
    d_l = _dev(torch, work, DC.padded_images([p[0] for p in pairs], ip, istr))
    d_r = _dev(torch, work, DC.padded_images([p[1] for p in pairs], ip, istr))
    d_d = _full(torch, work, 2 * n * dstr, 0x5A)
    d_z = _full(torch, work, 4 * n * zstr, 0x5A) if depth else None
    h.compute_batch_device(d_l, d_r, W, H, n, d_d, d_z, istr, ip, dstr, dp, zstr, zp)
    assert h.status() == 0
    disp, dpad = DC.unpadded(d_d.cpu().numpy().view(np.int16), n, H, W, dp, dstr)
    pad_kept = bool((d_d.cpu().numpy().view(np.int16).reshape(n, dstr)[dpad] == 0x5A5A).all())
    z = None
    if depth:
        zbuf = d_z.cpu().numpy().view(np.float32)
        z, zpad = DC.unpadded(zbuf, n, H, W, zp, zstr)
        pad_kept &= bool((zbuf.view(np.uint32).reshape(n, zstr)[zpad] == 0x5A5A5A5A).all())
    return disp, z, pad_kept


def _assert_equal(got_d, got_z, pair, what, **cfg):
    want_d, want_z = DC.ref(pair[0], pair[1], **cfg)
    print("%s: %d of %d disparities differ, valid share %.3f" % (what, int((got_d != want_d).sum()), want_d.size,
                                                                  (want_d > 0).mean()))
    assert got_d.tobytes() == want_d.tobytes(), what
    if got_z is not None:
        assert got_z.tobytes() == want_z.tobytes(), what


@pytest.mark.parametrize("seed", DC.SCENE_SEEDS)
def test_scene_equals_the_restatement(aria, torch_cuda, work, seed):
    """Shape (a): the synthetic scene at 200x96."""
    W, H = DC.SCENE
    pair = DC.scene_pair(seed, W, H)[:2]
    h = _handle(aria, work, DC.SCENE)
    try:
        d, z, _ = _run(torch_cuda, work, h, [pair])
        _assert_equal(d[0], z[0], pair, "scene %d" % seed)
        assert (d[0][:, 64:] > 0).mean() > 0.95
    finally:
        h.close()


@pytest.fixture(scope="module")
def noise_handle(aria, work):
    h = _handle(aria, work, DC.NOISE)
    yield h
    h.close()


@pytest.fixture(scope="module")
def batch_result(torch_cuda, work, noise_handle):
    """Shape (d)'s five pairs in one call on shape (b)'s padded layout."""
    return _run(torch_cuda, work, noise_handle, DC.batch_pairs(), padded=True)


def test_noise_pair_on_padded_layouts(batch_result):
    """Shape (b): 131x37 (W no multiple of 4), image pitch 160 with 0xA5 padding and a padded stride, disparity pitch 133
    (odd) and depth pitch 140 with padded strides, outputs prefilled 0x5A: no padding element changes. The noise pair holds
    valid pixels, ties, uniqueness failures and left-right failures."""
    d, z, pad_kept = batch_result
    pair = DC.batch_pairs()[0]
    _assert_equal(d[0], z[0], pair, "noise pair")
    assert pad_kept, "padding was written"
    want = DC.ref(*pair)[0]
    assert 0.1 < (want > 0).mean() < 0.7 and (want == -16).mean() > 0.3        # both kinds of pixel occur
    assert np.isfinite(z).all() and (z[d <= 0] == 0).all()


def test_narrow_and_constant_pairs(aria, torch_cuda, work):
    """Shape (c): 40x20, W < D, so most lanes of a pixel hold the constant cost; and a constant 70x9 pair (d16 = 0 on every
    pixel, see test_dense_host.py)."""
    W, H = DC.NARROW
    narrow = DC.scene_pair(3, W, H)[:2]
    const = DC.const_pair()
    h = _handle(aria, work, (max(W, DC.CONST[0]), max(H, DC.CONST[1])))
    try:
        d, z, _ = _run(torch_cuda, work, h, [narrow])
        _assert_equal(d[0], z[0], narrow, "40x20")
        d, z, _ = _run(torch_cuda, work, h, [const])
        _assert_equal(d[0], z[0], const, "constant 70x9")
        assert (d == 0).all() and (z == 0).all()
    finally:
        h.close()


def test_batch_independence_and_groups(aria, torch_cuda, work, noise_handle, batch_result):
    """Shape (d): five pairs in one call equal five calls of one pair and the blocking host form; a handle whose
    scratch_bytes admits two pairs in flight runs them as groups of 2, 2 and 1 with the same bytes."""
    from aria_slam_amd import dense
    pairs = DC.batch_pairs()
    d5, z5, pad_kept = batch_result
    assert pad_kept
    for k, pair in enumerate(pairs):
        _assert_equal(d5[k], z5[k], pair, "pair %d of the batch" % k)
        d1, z1, _ = _run(torch_cuda, work, noise_handle, [pair])
        assert d1[0].tobytes() == d5[k].tobytes() and z1[0].tobytes() == z5[k].tobytes(), k
    assert noise_handle.pairs_in_flight >= DC.N_BATCH
    dh, zh = noise_handle.compute(pairs[1][0], pairs[1][1])
    assert dh.tobytes() == d5[1].tobytes() and zh.tobytes() == z5[1].tobytes()
    assert noise_handle.compute(pairs[4][0], pairs[4][1], depth=False).tobytes() == d5[4].tobytes()
    per_pair = dense.scratch_bytes_per_pair(*DC.NOISE)
    h2 = _handle(aria, work, DC.NOISE, scratch_bytes=2 * per_pair + per_pair // 2)
    try:
        assert h2.pairs_in_flight == 2
        d, z, pad_kept = _run(torch_cuda, work, h2, pairs, padded=True)
        assert d.tobytes() == d5.tobytes() and z.tobytes() == z5.tobytes() and pad_kept
    finally:
        h2.close()


@pytest.mark.parametrize("cfg", DC.PARAM_SETS, ids=["P1=1,P2=127", "uniqueness=0", "lr=-1", "lr=0"])
def test_parameters(aria, torch_cuda, work, cfg):
    """Shape (e): non-default parameters on shape (b)'s noise pair and one scene pair."""
    pairs = DC.batch_pairs()[:2]
    h = _handle(aria, work, DC.NOISE, **cfg)
    try:
        d, z, _ = _run(torch_cuda, work, h, pairs)
        for k, pair in enumerate(pairs):
            _assert_equal(d[k], z[k], pair, "%r pair %d" % (cfg, k), **cfg)
    finally:
        h.close()
    if cfg.get("lr_max_diff", 0) < 0 or "uniqueness" in cfg:                   # the rule that was switched off mattered
        assert (DC.ref(*pairs[0], **cfg)[0] > 0).sum() > (DC.ref(*pairs[0])[0] > 0).sum()


def test_sampling(aria, torch_cuda, work, noise_handle, batch_result):
    """Shape (f): three frames with counts 0, 1 and kp_stride on the device's maps of the first three pairs of the batch
    (disparity pitch 133); keypoints that round outside the image, on invalid pixels, NaN and huge; records beyond the count
    are unmatched; a count of kp_stride + 1 skips its frame and is reported once."""
    from aria_slam_amd import dense_ref as R
    from aria_slam_amd._lib import STEREO_OBS_DTYPE
    torch = torch_cuda
    W, H = DC.NOISE
    kp, counts = DC.sample_keypoints()
    maps = batch_result[0][:3]
    d_disp = _dev(torch, work, _pitched_maps(maps))
    for cnt in (counts, np.array([DC.KP_STRIDE, DC.KP_STRIDE + 1, -1], np.int32)):
        d_kp, d_n = _dev(torch, work, kp), _dev(torch, work, cnt)
        d_obs = _full(torch, work, 3 * DC.KP_STRIDE * 32, 0x5A)
        noise_handle.sample_batch_device(d_disp, W, H, d_kp, d_n, DC.KP_STRIDE, 3, d_obs, DC.DISP_STRIDE, DC.DISP_PITCH)
        bad = bool(((cnt < 0) | (cnt > DC.KP_STRIDE)).any())
        assert noise_handle.status() == (-1 if bad else 0)                    # ARIA_E_INVALID, once
        assert noise_handle.status() == 0
        got = d_obs.cpu().numpy().view(STEREO_OBS_DTYPE).reshape(3, DC.KP_STRIDE)
        want = R.sample_batch(maps, kp, cnt, DC.K, DC.BASELINE)
        assert got.tobytes() == want.tobytes()
    want = R.sample_batch(maps, kp, counts, DC.K, DC.BASELINE)
    matched = want["right_idx"] == R.NO_KEYPOINT
    assert matched[2].sum() >= 8 and (~matched[2]).sum() >= 8 and not matched[0].any() and not matched[1, 1:].any()
    inside = (np.rint(kp["x"][2]) >= 0) & (np.rint(kp["x"][2]) <= W - 1) & (np.rint(kp["y"][2]) >= 0) & (np.rint(kp["y"][2]) <= H - 1)
    assert (inside & ~matched[2]).any() and (~inside).sum() >= 4              # on invalid pixels, and outside the image
    assert np.isfinite(np.stack([want[f] for f in ("u_right", "disparity", "depth", "X", "Y")])).all()
    # the blocking host form
    assert noise_handle.sample(maps[2], kp[2]).tobytes() == want[2].tobytes()


def _pitched_maps(maps):
    n, H, W = maps.shape
    buf = np.full((n, DC.DISP_STRIDE), 0x5A5A, np.int16)
    for k in range(n):
        buf[k, :DC.DISP_PITCH * H].reshape(H, DC.DISP_PITCH)[:, :W] = maps[k]
    return buf


def test_chain_raw_pair_to_metric_scale(aria, torch_cuda, work):
    """Shape (g): two raw synthetic pairs at 320x240 -> device remap of both cameras -> aria_dense_compute_batch_device ->
    aria_dense_sample_batch_device on the device extractor's keypoints of the rectified left images ->
    aria_stereo_scale_batch_device with pair 0's records as the query side and pair 1's as the train side of a synthetic
    pose. Nothing leaves HBM in between, and every stage's output equals its restatement on the previous stage's device
    output."""
    from aria_slam_amd import dense_ref as R
    from aria_slam_amd import rectify_ref as RR
    from aria_slam_amd import stereo_ref as SR
    from aria_slam_amd._lib import KP_DTYPE, MATCH_DTYPE, POSE_RESULT_DTYPE, STEREO_OBS_DTYPE, STEREO_SCALE_DTYPE
    import rectify_cases as RC
    torch = torch_cuda
    W, H, NF, n = 320, 240, 500, 2
    cal = RR.scaled_calibration(W, H, RC.EUROC)
    pairs = [RR.raw_stereo_pair(seed, W, H, cal) for seed in (1, 2)]
    cl, cr, nk, baseline = RR.rectified_cameras(cal)
    r = aria.HipRectifier.from_stereo_calibration(cal["K_l"], cal["D_l"], cal["T_BS_l"], cal["K_r"], cal["D_r"], cal["T_BS_r"],
                                                  (W, H), stream=work.cuda_stream)
    e = aria.OrbHipExtractor(max_features=NF, stream=work.cuda_stream, max_width=W, max_height=H, max_batch=n)
    dn = aria.HipDenseStereo(K=r.new_K, baseline=r.baseline, max_size=(W, H), stream=work.cuda_stream)
    st = aria.HipStereoMatcher(K=r.new_K, baseline=r.baseline, stream=work.cuda_stream)
    try:
        cap = e.kp_capacity()
        rect = []
        for cam in (0, 1):
            d_raw = _dev(torch, work, np.stack([p[cam] for p in pairs]))
            d_img = _full(torch, work, n * W * H, 0x5A)
            r.remap_batch_device(d_raw, n, d_img, cam)
            rect.append(d_img)
        d_kp, d_desc = _full(torch, work, n * cap * 24, 0), _full(torch, work, n * cap * 32, 0)
        d_n = _full(torch, work, 4 * n, 0).view(torch.int32)
        assert r.status() == 0
        e.extract_batch_device(rect[0], n, W, H, d_kp, d_desc, d_n, cap)
        e.check()
        d_disp, d_z = _full(torch, work, 2 * n * W * H, 0x5A), _full(torch, work, 4 * n * W * H, 0x5A)
        dn.compute_batch_device(rect[0], rect[1], W, H, n, d_disp, d_z)
        d_obs = _full(torch, work, n * cap * 32, 0x5A)
        dn.sample_batch_device(d_disp, W, H, d_kp, d_n, cap, n, d_obs)
        assert dn.status() == 0
        nl = d_n.cpu().numpy()
        n_id = int(nl.min())
        rec = np.zeros(1, POSE_RESULT_DTYPE)
        rec["R"], rec["t"], rec["valid"] = np.eye(3).reshape(-1), [1.0, 0.0, 0.0], 1
        ident = np.zeros(cap, MATCH_DTYPE)
        ident["query_idx"][:n_id] = ident["train_idx"][:n_id] = np.arange(n_id)
        d_rec, d_ident = _dev(torch, work, rec), _dev(torch, work, ident)
        d_nid = _dev(torch, work, np.array([n_id], np.int32))
        d_scale = _full(torch, work, 16, 0x5A)
        st.scale_batch_device(d_rec, None, d_ident, d_nid, cap, d_obs, d_n, d_obs.data_ptr() + cap * 32, d_n.data_ptr() + 4, cap, 1,
                              d_scale)
        assert st.status() == 0
        # every stage against its restatement on the previous stage's device output
        imgs = [t.cpu().numpy().reshape(n, H, W) for t in rect]
        for idx, cam in ((0, cl), (1, cr)):
            want = np.stack([RR.remap(p[idx], RR.build_map(cam, nk, W, H, W, H)) for p in pairs])
            assert imgs[idx].tobytes() == want.tobytes(), idx
        disp = d_disp.cpu().numpy().view(np.int16).reshape(n, H, W)
        z = d_z.cpu().numpy().view(np.float32).reshape(n, H, W)
        for p in range(n):
            want_d = R.dense_disparity(imgs[0][p], imgs[1][p])
            assert disp[p].tobytes() == want_d.tobytes(), p
            assert z[p].tobytes() == R.depth_map(want_d, r.new_K, r.baseline).tobytes(), p
        kp = d_kp.cpu().numpy().view(KP_DTYPE).reshape(n, cap)
        obs = d_obs.cpu().numpy().view(STEREO_OBS_DTYPE).reshape(n, cap)
        want_obs = R.sample_batch(disp, kp, nl, r.new_K, r.baseline)
        assert obs.tobytes() == want_obs.tobytes()
        for p in range(n):
            with_depth = int((obs[p, :nl[p]]["right_idx"] == R.NO_KEYPOINT).sum())
            print("pair %d: %d of %d keypoints get a depth, valid share of the map %.3f" % (p, with_depth, nl[p], (disp[p] > 0).mean()))
            assert with_depth > 0.5 * nl[p] and nl[p] > 256
        got_scale = d_scale.cpu().numpy().view(STEREO_SCALE_DTYPE)[0]
        want_scale = SR.stereo_scale_ref(rec[0], None, ident[:n_id], obs[0, :nl[0]], obs[1, :nl[1]])
        assert got_scale.tobytes() == want_scale.tobytes()
        assert got_scale["n_used"] > 0.25 * n_id
    finally:
        st.close()
        dn.close()
        e.close()
        r.close()


def test_lifecycle_and_refusals(aria, torch_cuda, work):
    """Shape (h): create and destroy on a borrowed stream and on an owned one; num_disparities = 128, P1 > P2 and a
    scratch_bytes too small for one pair are refused; a pair larger than max_size is refused by the call."""
    from aria_slam_amd import dense
    torch = torch_cuda
    pair = DC.noise_pair(7)
    want = DC.ref(*pair)[0]
    borrowed = _handle(aria, work, DC.NOISE)
    assert borrowed.stream == work.cuda_stream
    assert borrowed.compute(pair[0], pair[1], depth=False).tobytes() == want.tobytes()
    borrowed.close()
    borrowed.close()                                                           # idempotent
    work.synchronize()                                                         # the borrowed stream is still the caller's
    owned = aria.HipDenseStereo(K=DC.K, baseline=DC.BASELINE, max_size=DC.NOISE)
    assert owned.stream and owned.stream != work.cuda_stream
    assert owned.compute(pair[0], pair[1], depth=False).tobytes() == want.tobytes()
    with pytest.raises(aria.AriaError) as err:
        owned.compute(np.zeros((DC.NOISE[1] + 1, DC.NOISE[0]), np.uint8), np.zeros((DC.NOISE[1] + 1, DC.NOISE[0]), np.uint8))
    assert err.value.status == -1
    owned.close()
    for kw in (dict(num_disparities=128), dict(P1=33, P2=32), dict(scratch_bytes=dense.scratch_bytes_per_pair(*DC.NOISE) - 1)):
        with pytest.raises(aria.AriaError) as err:
            _handle(aria, work, DC.NOISE, **kw)
        assert err.value.status == -1, kw                                      # ARIA_E_INVALID
    one = _handle(aria, work, DC.NOISE, scratch_bytes=dense.scratch_bytes_per_pair(*DC.NOISE))
    assert one.pairs_in_flight == 1
    one.close()
    torch.cuda.synchronize()
