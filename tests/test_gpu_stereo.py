"""Sparse stereo on the MI355X (aria_stereo_*, kernels in aria_slam_amd/csrc/stereo_match.hip) against its definition, the
NumPy restatement aria_slam_amd/stereo_ref.py: every field of every aria_stereo_obs record, the match lists, the counts
and aria_stereo_scale are BITWISE equal. A difference in an fp32 or fp64 field is a contraction or ordering bug, never a
tolerance."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stereo_cases   # noqa: E402

W, H, NF = 320, 240, 500
PITCH = 352                                  # != W
IMG_STRIDE = PITCH * H + 64                  # padded


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
        t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to("cuda:0")
    work.synchronize()
    return t


def _zeros(torch, work, nbytes):
    with torch.cuda.stream(work):
        t = torch.zeros(max(nbytes, 1), dtype=torch.uint8, device="cuda:0")
    work.synchronize()
    return t


def _padded(imgs, pitch, stride):
    out = np.full((len(imgs), stride), 0xA5, np.uint8)           # the padding is not zero: nobody may read it
    for p, im in enumerate(imgs):
        h, w = im.shape
        rows = out[p, :pitch * h].reshape(h, pitch)
        rows[:, :w] = im
    return out


def _run_match(aria, torch, work, st, d_il, d_ir, img_stride, w, h, pitch, d_kl, d_dl, d_nl, d_kr, d_dr, d_nr, cap, n):
    """aria_stereo_match_batch_device on device tensors -> host (obs (n, cap), matches (n, cap), counts (n,), status)."""
    from aria_slam_amd._lib import MATCH_DTYPE, STEREO_OBS_DTYPE
    with torch.cuda.stream(work):
        obs = torch.full((n * cap * 32,), 0x5A, dtype=torch.uint8, device="cuda:0")
        m = torch.full((n * cap * 12,), 0x5A, dtype=torch.uint8, device="cuda:0")
        nm = torch.full((n,), -7, dtype=torch.int32, device="cuda:0")
    work.synchronize()
    st.match_batch_device(d_il, d_ir, img_stride, w, h, pitch, d_kl, d_dl, d_nl, d_kr, d_dr, d_nr, cap, n, obs, m, nm)
    status = st.status()
    return (obs.cpu().numpy().view(STEREO_OBS_DTYPE).reshape(n, cap), m.cpu().numpy().view(MATCH_DTYPE).reshape(n, cap),
            nm.cpu().numpy(), status)


def _assert_pair_equal(tag, obs, m, nm, want_obs, want_m):
    """One pair: obs (cap records), m (cap rows), nm against the restatement's (n_left records, matches)."""
    from aria_slam_amd import stereo_ref as R
    full = R.unmatched_obs(len(obs))
    full[:len(want_obs)] = want_obs
    if obs.tobytes() != full.tobytes():
        for f in obs.dtype.names:
            bad = np.flatnonzero(obs[f].view(np.int32) != full[f].view(np.int32))
            if len(bad):
                print("%s: field %s differs at %s: got %s want %s" % (tag, f, bad[:8], obs[f][bad[:8]], full[f][bad[:8]]))
    assert obs.tobytes() == full.tobytes(), tag
    assert nm == len(want_m), (tag, nm, len(want_m))
    assert m[:nm].tobytes() == want_m.tobytes(), tag


@pytest.fixture(scope="module")
def scene(aria, torch_cuda, work):
    """Shape (a): three pairs at 320x240 / 500 features from the device extractor -- seeds 1 and 2 and a pair whose right
    frame is blank (0 keypoints) -- with pitch != W and a padded image stride; the restatement of each, computed once."""
    from aria_slam_amd import stereo_ref as R
    from aria_slam_amd._lib import KP_DTYPE
    torch = torch_cuda
    pairs = [R.stereo_pair(1, W, H), R.stereo_pair(2, W, H), R.stereo_pair(3, W, H)]
    lefts = [p[0] for p in pairs]
    rights = [pairs[0][1], pairs[1][1], np.full((H, W), 110, np.uint8)]
    d_il = _dev(torch, work, _padded(lefts, PITCH, IMG_STRIDE))
    d_ir = _dev(torch, work, _padded(rights, PITCH, IMG_STRIDE))
    e = aria.OrbHipExtractor(max_features=NF, stream=work.cuda_stream, max_width=W, max_height=H, max_batch=3)
    cap = e.kp_capacity()
    side = []
    for d_img in (d_il, d_ir):
        k, d, c = _zeros(torch, work, 3 * cap * 24), _zeros(torch, work, 3 * cap * 32), _zeros(torch, work, 12).view(torch.int32)
        e.extract_batch_device(d_img, 3, W, H, k, d, c, cap, frame_stride=IMG_STRIDE, row_stride=PITCH)
        e.check()
        side.append((k, d, c))
    e.close()
    (d_kl, d_dl, d_nl), (d_kr, d_dr, d_nr) = side
    nl, nr = d_nl.cpu().numpy(), d_nr.cpu().numpy()
    kl = d_kl.cpu().numpy().view(KP_DTYPE).reshape(3, cap)
    kr = d_kr.cpu().numpy().view(KP_DTYPE).reshape(3, cap)
    dl, dr = d_dl.cpu().numpy().reshape(3, cap, 32), d_dr.cpu().numpy().reshape(3, cap, 32)
    assert nr[2] == 0 and nl[0] % 64 and nl[1] % 64 and nl[2] % 64 and min(nl) > 256
    host = [(lefts[p], rights[p], kl[p, :nl[p]].copy(), dl[p, :nl[p]].copy(), kr[p, :nr[p]].copy(), dr[p, :nr[p]].copy())
            for p in range(3)]
    want = [R.stereo_match_ref(*host[p]) for p in range(3)]
    return dict(dev=(d_il, d_ir, IMG_STRIDE, W, H, PITCH, d_kl, d_dl, d_nl, d_kr, d_dr, d_nr, cap, 3), cap=cap, host=host,
                want=want, nl=nl, nr=nr)


def test_extracted_pairs_equal_the_restatement(aria, torch_cuda, work, scene):
    st = aria.HipStereoMatcher(stream=work.cuda_stream)
    try:
        obs, m, nm, status = _run_match(aria, torch_cuda, work, st, *scene["dev"])
        assert status == 0
        for p in range(3):
            _assert_pair_equal("pair %d" % p, obs[p], m[p], nm[p], *scene["want"][p])
        assert nm[0] > 250 and nm[1] > 250 and nm[2] == 0             # most of ~465 left keypoints get a depth
        assert np.isfinite(np.stack([obs[f] for f in ("u_right", "disparity", "depth", "X", "Y")])).all()
    finally:
        st.close()


@pytest.mark.parametrize("cfg", [stereo_cases.CFG_BOUNDS, stereo_cases.CFG_DEFAULT], ids=["bounds", "default"])
def test_rule_cases_as_one_batch(aria, torch_cuda, work, cfg):
    """Shape (b): the hand-made cases of tests/test_stereo_host.py, those of one configuration as one batch."""
    from aria_slam_amd import stereo_ref as R
    torch = torch_cuda
    cases = [c for c in stereo_cases.rule_cases() if c["cfg"] == cfg]
    cap = 16
    il, ir, kl, kr, dl, dr, nl, nr = stereo_cases.stack_cases(cases, cap)
    cw, ch = stereo_cases.W, stereo_cases.H
    st = aria.HipStereoMatcher(stream=work.cuda_stream, **cfg)
    try:
        args = [_dev(torch, work, a) for a in (il, ir)] + [cw * ch, cw, ch, cw] + \
               [_dev(torch, work, a) for a in (kl, dl, nl, kr, dr, nr)] + [cap, len(cases)]
        obs, m, nm, status = _run_match(aria, torch, work, st, *args)
        assert status == 0
        for p, c in enumerate(cases):
            want = R.stereo_match_ref(c["img_l"], c["img_r"], c["kp_l"], c["desc_l"], c["kp_r"], c["desc_r"], **c["cfg"])
            _assert_pair_equal(c["name"], obs[p], m[p], nm[p], *want)
            for i, e in enumerate(c["expect"]):
                assert (obs[p][i]["right_idx"] if e else -1) == (e[0] if e else -1), (c["name"], i)
    finally:
        st.close()


@pytest.mark.parametrize("w,L", [(3, 8), (7, 16)])
def test_window_and_slide_sizes(aria, torch_cuda, work, scene, w, L):
    """Shape (c): a 7x7 window slid over 17 shifts (two passes of the 16 lanes) and the largest, 15x15 over 33 (three)."""
    from aria_slam_amd import stereo_ref as R
    st = aria.HipStereoMatcher(stream=work.cuda_stream, sad_half_window=w, sad_slide=L)
    try:
        obs, m, nm, status = _run_match(aria, torch_cuda, work, st, *scene["dev"])
        assert status == 0
        for p in range(3):
            want = R.stereo_match_ref(*scene["host"][p], sad_half_window=w, sad_slide=L)
            _assert_pair_equal("w=%d L=%d pair %d" % (w, L, p), obs[p], m[p], nm[p], *want)
        assert nm[0] > 100 and nm[1] > 100 and nm[2] == 0
    finally:
        st.close()


def test_batch_equals_single_calls_and_is_reproducible(aria, torch_cuda, work, scene):
    """Shape (d): the batch of three equals three blocking one-pair calls on host buffers; two runs are bitwise equal."""
    st = aria.HipStereoMatcher(stream=work.cuda_stream)
    try:
        a = _run_match(aria, torch_cuda, work, st, *scene["dev"])
        b = _run_match(aria, torch_cuda, work, st, *scene["dev"])
        for x, y in zip(a[:3], b[:3]):
            assert x.tobytes() == y.tobytes()
        for p in range(3):
            il, ir, kl, dl, kr, dr = scene["host"][p]
            pad = np.zeros((2, H, PITCH), np.uint8)
            pad[0, :, :W], pad[1, :, :W] = il, ir
            obs, m = st.match(pad[0, :, :W], pad[1, :, :W], (kl, dl), (kr, dr))   # strided views: pitch != W on the host too
            assert obs.tobytes() == a[0][p][:len(kl)].tobytes() and m.tobytes() == a[1][p][:a[2][p]].tobytes()
    finally:
        st.close()


def test_bad_count_skips_only_that_pair(aria, torch_cuda, work, scene):
    """Shape (e): a count of kp_stride + 1 -> that pair is skipped, aria_stereo_check returns ARIA_E_INVALID once, the others
    are intact."""
    from aria_slam_amd import stereo_ref as R
    torch = torch_cuda
    dev = list(scene["dev"])
    cap = scene["cap"]
    nl = scene["nl"].copy()
    nl[1] = cap + 1
    dev[8] = _dev(torch, work, nl).view(torch.int32)
    st = aria.HipStereoMatcher(stream=work.cuda_stream)
    try:
        obs, m, nm, status = _run_match(aria, torch, work, st, *dev)
        assert status == -1 and st.status() == 0                     # ARIA_E_INVALID, reported once
        for p in (0, 2):
            _assert_pair_equal("pair %d" % p, obs[p], m[p], nm[p], *scene["want"][p])
        assert nm[1] == 0 and obs[1].tobytes() == R.unmatched_obs(cap).tobytes()
        with pytest.raises(aria.AriaError):
            st.match_batch_device(*dev[:12], 8193, 3, dev[0], dev[0], dev[0])       # kp_stride beyond the LDS bound
    finally:
        st.close()


def test_match_list_feeds_the_mapper_on_the_device(aria, torch_cuda, work, scene):
    """Shape (f), first half: the compacted match list goes to aria_map_triangulate_batch_device unchanged, with extrinsics
    [I|0], [I|(-baseline, 0, 0)], no host copy in between. With a 0.11 m baseline the mapper's 1 degree parallax gate passes
    depths below 6.3 m: the rows of 19.5 and 42.25 px disparity (2.6 m and 1.2 m), not those of 7 px (7.2 m)."""
    from aria_slam_amd._lib import MATCH_DTYPE, STEREO_OBS_DTYPE
    torch = torch_cuda
    d_il, d_ir, stride, w, h, pitch, d_kl, d_dl, d_nl, d_kr, d_dr, d_nr, cap, n = scene["dev"]
    b = 0.110
    ext = np.tile(np.concatenate([np.eye(3, 4).ravel(), np.concatenate([np.eye(3), [[-b], [0], [0]]], 1).ravel()]), (n, 1))
    d_ext = _dev(torch, work, ext)
    obs, m, nm = _zeros(torch, work, n * cap * 32), _zeros(torch, work, n * cap * 12), _zeros(torch, work, 4 * n).view(torch.int32)
    added = _zeros(torch, work, 4 * n).view(torch.int32)
    st = aria.HipStereoMatcher(stream=work.cuda_stream, baseline=b)
    mp = aria.HipMapper(stream=work.cuda_stream)
    try:
        st.match_batch_device(d_il, d_ir, stride, w, h, pitch, d_kl, d_dl, d_nl, d_kr, d_dr, d_nr, cap, n, obs, m, nm)
        mp.triangulate_batch_device(d_kl, d_nl, d_kr, d_nr, cap, m, nm, n, cap, d_extrinsics=d_ext, d_img=d_il, img_stride=stride,
                                    width=w, height=h, pitch=pitch, d_added=added)
        st.check()
        mp.check()
        pts = mp.read()
        add = added.cpu().numpy()
        assert add[0] > 50 and add[1] > 50 and add[2] == 0 and len(pts) == add.sum()
        o = obs.cpu().numpy().view(STEREO_OBS_DTYPE).reshape(n, cap)
        mh = m.cpu().numpy().view(MATCH_DTYPE).reshape(n, cap)
        # every map point is a stereo match of its pair, and the two depths agree: the mapper triangulates the right KEYPOINT,
        # the stereo stage the sub-pixel SAD position at most sad_slide - 1 + 0.5 px from it, on disparities >= 19 px
        assert np.array_equal(pts["idx1"], mh[pts["pair"], pts["match"]]["query_idx"])
        assert np.array_equal(pts["idx2"], mh[pts["pair"], pts["match"]]["train_idx"])
        depth = o[pts["pair"], pts["idx1"]]["depth"]
        assert (depth > 0).all() and np.median(np.abs(pts["X"][:, 2] - depth) / depth) < 4.5 / 19.0
    finally:
        mp.close()
        st.close()


def _sequence(n_frames=4, n=300, seed=5):
    """A synthetic stereo sequence without images: world points seen by a moving rig. Per frame the left keypoints (fp32
    pixels) and the stereo observations (camera-frame X, Y, depth as fp32, every keypoint matched)."""
    from aria_slam_amd import map_ref as M
    from aria_slam_amd import stereo_ref as R
    from aria_slam_amd._lib import KP_DTYPE, MATCH_DTYPE
    fx, fy, cx, cy = R.EUROC_K
    rng = np.random.default_rng(seed)
    Xw = np.stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(3, 10, n)], 1)
    kps, obs, poses = np.zeros((n_frames, n), KP_DTYPE), [], []
    for f in range(n_frames):
        Rf, tf = M.rot([0.1, 1, 0.05], 2.0 * f), np.array([0.30, 0.05, 0.10]) * f * (1 + 0.2 * f)
        Xc = Xw @ Rf.T + tf
        kps[f]["x"], kps[f]["y"] = fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy
        kps[f]["size"], kps[f]["response"] = 31.0, 1.0
        o = R.unmatched_obs(n)
        o["X"], o["Y"], o["depth"], o["right_idx"] = Xc[:, 0], Xc[:, 1], Xc[:, 2], np.arange(n)
        obs.append(o)
        poses.append((Rf, tf))
    rel = []                                                          # x_{f+1} = Rr x_f + tr
    for f in range(n_frames - 1):
        Rr = poses[f + 1][0] @ poses[f][0].T
        rel.append((Rr, poses[f + 1][1] - Rr @ poses[f][1]))
    m = np.zeros(n, MATCH_DTYPE)
    m["query_idx"] = m["train_idx"] = np.arange(n)
    return kps, np.stack(obs), m, rel


def _max_norm(o):
    return np.sqrt(o["X"].astype(np.float64) ** 2 + o["Y"].astype(np.float64) ** 2 + o["depth"].astype(np.float64) ** 2).max()


def test_scale_of_pose_records_on_the_device(aria, torch_cuda, work):
    """Shape (f), second half: the pose stage's records and masks of a 4-frame sequence are scaled where they lie:
    valid = 1, bitwise the restatement's, and the metric length of each step as far as the pose record allows. With
    X2 = R X1 + s t and the record's (R^, t^): s_m - s = s (t^.t - 1) + t^.(R - R^) X1, so
    |scale - s| <= s (1 - t^.t) + |R - R^|_2 max |X1| + the fp32 storage of the points (1e-5).
    Then the deferred error of an out-of-range match index, and the blocking host form."""
    from aria_slam_amd import stereo_ref as R
    from aria_slam_amd._lib import POSE_RESULT_DTYPE, STEREO_SCALE_DTYPE
    torch = torch_cuda
    kps, obs, m, rel = _sequence()
    B, n = kps.shape
    cap = n + 20                                                      # strides larger than the counts
    kp_pad, obs_pad = np.zeros((B, cap), kps.dtype), np.zeros((B, cap), obs.dtype)
    kp_pad[:, :n], obs_pad[:, :n] = kps, obs
    obs_pad[1, 7:19] = R.unmatched_obs(1)[0]                          # some keypoints of frame 1 have no depth
    mm = np.zeros((B - 1, cap), m.dtype)
    mm[:, :n] = m
    d_kp, d_obs, d_m = (_dev(torch, work, a) for a in (kp_pad, obs_pad, mm))
    d_cnt = _dev(torch, work, np.full(B, n, np.int32)).view(torch.int32)
    d_nm = _dev(torch, work, np.full(B - 1, n, np.int32)).view(torch.int32)
    d_pose, d_mask = _zeros(torch, work, (B - 1) * 192), _zeros(torch, work, (B - 1) * cap)
    d_out = _zeros(torch, work, (B - 1) * 16)
    pe = aria.HipPoseEstimator(stream=work.cuda_stream)
    st = aria.HipStereoMatcher(stream=work.cuda_stream)
    try:
        # view 1 = train = frame p, view 2 = query = frame p + 1
        q = lambda t, rec: t.data_ptr() + cap * rec                   # noqa: E731
        pe.estimate_batch_device(q(d_kp, 24), d_cnt.data_ptr() + 4, d_kp, d_cnt, cap, d_m, d_nm, B - 1, cap, d_pose, d_mask,
                                 query_is_first=False)
        st.scale_batch_device(d_pose, d_mask, d_m, d_nm, cap, q(d_obs, 32), d_cnt.data_ptr() + 4, d_obs, d_cnt, cap, B - 1, d_out,
                              query_is_first=False)
        pe.check()
        st.check()
        got = d_out.cpu().numpy().view(STEREO_SCALE_DTYPE)
        rec = d_pose.cpu().numpy().view(POSE_RESULT_DTYPE)
        mask = d_mask.cpu().numpy().reshape(B - 1, cap)
        for p in range(B - 1):
            want = R.stereo_scale_ref(rec[p], mask[p, :n], m, obs_pad[p + 1, :n], obs_pad[p, :n], query_is_first=False)
            assert got[p].tobytes() == want.tobytes(), (p, got[p], want)
            assert got[p]["valid"] == 1 and got[p]["n_used"] > n // 2   # noise-free matches are inliers of the true E
            Rr, tr = rel[p]
            s_true = np.linalg.norm(tr)
            bound = s_true * (1.0 - rec[p]["t"] @ (tr / s_true)) + \
                np.linalg.norm(Rr - rec[p]["R"].reshape(3, 3), 2) * _max_norm(obs[p]) + 1e-5
            print("pair %d: scale %.9f true %.9f bound %.3g" % (p, got[p]["scale"], s_true, bound))
            assert abs(got[p]["scale"] - s_true) <= bound
            single = st.scale(rec[p], m, obs_pad[p + 1, :n], obs_pad[p, :n], mask=mask[p, :n], query_is_first=False)
            assert single.tobytes() == want.tobytes()
        # an invalid pose record and an out-of-range index
        bad_m = mm.copy()
        bad_m[1, 3]["train_idx"] = n
        rec2 = rec.copy()
        rec2[0]["valid"] = 0
        st.scale_batch_device(_dev(torch, work, rec2), d_mask, _dev(torch, work, bad_m), d_nm, cap, q(d_obs, 32),
                              d_cnt.data_ptr() + 4, d_obs, d_cnt, cap, B - 1, d_out, query_is_first=False)
        assert st.status() == -1 and st.status() == 0
        got2 = d_out.cpu().numpy().view(STEREO_SCALE_DTYPE)
        for p in (0, 1):
            assert (got2[p]["scale"], got2[p]["n_used"], got2[p]["valid"]) == (1.0, 0, 0)
        assert got2[2].tobytes() == got[2].tobytes()
    finally:
        st.close()
        pe.close()
