"""Rectification on the MI355X (aria_rect_*, kernels in aria_slam_amd/csrc/rectify.hip) against its definition, the NumPy
restatement aria_slam_amd/rectify_ref.py: every map word, every pixel and every keypoint field is BITWISE equal. A
difference in a map word or in an fp32 coordinate is a contraction or ordering bug, never a tolerance.

Shapes (a)-(e) are one calibration at one source size. The cases of rectify_cases.EDGE_CASES add what they leave out: both
sides of every term of k_rect_remap's choice between its read forms, three frame groups with a short last one, rotations far
from the identity with k3 != 0 and Z <= 0, sources down to 2x2, a destination narrower than a lane and the 2047 limit of the
map word; tests/test_rectify_host.py asserts that each case reaches its branch. The same cases run through the kernel text
compiled for the host in tests/test_rectify_kernel_emulation.py: a case that fails here and passes there is a difference in
the device's arithmetic, one that fails in both is an indexing bug."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rectify_cases as RC   # noqa: E402


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


def _rectifier(aria, work, small, **kw):
    return aria.HipRectifier.from_stereo_calibration(RC.K_L, RC.D_L, RC.T_BS_L, RC.K_R, RC.D_R, RC.T_BS_R, RC.SIZE,
                                                     RC.SMALL if small else None, RC.SMALL_NEW_K if small else None,
                                                     stream=work.cuda_stream, **kw)


@pytest.fixture(scope="module")
def small_rect(aria, work):
    r = _rectifier(aria, work, True, fill=RC.FILL)
    yield r
    r.close()


@pytest.mark.parametrize("small", [False, True], ids=["752x480", "637x399"])
def test_maps_equal_the_restatement(aria, work, small):
    """Shape (a): both cameras of the stereo calibration, 752x480 -> 752x480 with the default new K and -> 637x399 (W no
    multiple of 4, an invalid border, every fraction value)."""
    from aria_slam_amd import rectify_ref as R
    r = _rectifier(aria, work, small)
    try:
        cl, cr, nk, baseline = RC.cameras(RC.SMALL_NEW_K if small else None)
        assert r.new_K == nk and r.baseline == baseline
        assert r.camera(0) == cl and r.camera(1) == cr
        for k in range(2):
            want = RC.ref_maps(small)[k]
            got = r.map(k)
            share = (want == R.INVALID).mean()
            print("camera %d: %.1f %% invalid, %d words differ" % (k, 100 * share, int((got != want).sum())))
            if small:
                assert 0.10 < share < 0.30                       # neither empty nor fully invalid
            assert got.tobytes() == want.tobytes(), (small, k)
        assert r.status() == 0
    finally:
        r.close()


def _remap_batch(torch, work, r, cam, frames):
    """The batch form on shape (b)'s layout -> (images (n, 399, 637), True when no padding byte changed)."""
    n = len(frames)
    d_src = _dev(torch, work, RC.padded(frames, RC.SRC_PITCH, RC.SRC_STRIDE))
    d_dst = _full(torch, work, n * RC.DST_STRIDE, 0x5A)
    r.remap_batch_device(d_src, n, d_dst, cam, RC.SRC_STRIDE, RC.SRC_PITCH, RC.DST_STRIDE, RC.DST_PITCH)
    assert r.status() == 0
    buf = d_dst.cpu().numpy()
    img, is_pad = RC.unpadded(buf, n, RC.SMALL[1], RC.SMALL[0], RC.DST_PITCH, RC.DST_STRIDE)
    return img, bool((buf.reshape(n, RC.DST_STRIDE)[is_pad] == 0x5A).all())


@pytest.fixture(scope="module")
def batch_results(torch_cuda, work, small_rect):
    return [_remap_batch(torch_cuda, work, small_rect, k, RC.noise_frames()[k]) for k in range(2)]


def test_remap_equals_the_restatement(batch_results):
    """Shape (b): 637x399, five frames of uniform noise, source pitch 768 with 0xA5 padding and a padded stride, destination
    pitch 641 (odd: unaligned rows) with a padded stride prefilled 0x5A, fill = 7, both cameras."""
    for k, (img, pad_kept) in enumerate(batch_results):
        want = RC.ref_remapped()[k]
        print("camera %d: %d of %d pixels differ" % (k, int((img != want).sum()), want.size))
        assert img.tobytes() == want.tobytes(), k
        assert pad_kept, "padding was written"
    assert (RC.ref_remapped() == RC.FILL).mean() > 0.10


def test_batch_independence_and_host_form(torch_cuda, work, small_rect, batch_results):
    """Shape (c): five frames in one call equal five calls of one frame, and the blocking host form equals both."""
    frames = RC.noise_frames()[1]
    for f in range(RC.N_FRAMES):
        img, pad_kept = _remap_batch(torch_cuda, work, small_rect, 1, frames[f:f + 1])
        assert img.tobytes() == batch_results[1][0][f:f + 1].tobytes() and pad_kept, f
    for f in (0, RC.N_FRAMES - 1):
        assert small_rect.remap(frames[f], 1).tobytes() == batch_results[1][0][f].tobytes(), f
    pitched = RC.padded(RC.noise_frames()[0][:1], RC.SRC_PITCH, RC.SRC_STRIDE)[0, :RC.SRC_PITCH * 480].reshape(480, RC.SRC_PITCH)
    assert small_rect.remap(pitched[:, :752], 0).tobytes() == batch_results[0][0][0].tobytes()   # a pitched host image


def test_points_equal_the_restatement(aria, torch_cuda, work):
    """Shape (d): three frames with counts 0, 1 and kp_stride = 300, keypoints out to the image corners; in place equals out
    of place; every other field unchanged; a count of kp_stride + 1 skips its frame and is reported once."""
    torch = torch_cuda
    kp, counts = RC.keypoints()
    r = _rectifier(aria, work, False)
    try:
        for cam in range(2):
            want = RC.ref_points(cam, kp, counts)
            d_in, d_n = _dev(torch, work, kp), _dev(torch, work, counts)
            d_out = _full(torch, work, kp.nbytes, 0x5A)
            r.points_batch_device(d_in, d_n, RC.KP_STRIDE, 3, d_out, cam)
            assert r.status() == 0
            out = d_out.cpu().numpy().view(kp.dtype).reshape(kp.shape)
            for f, n in enumerate(counts):
                assert out[f, :n].tobytes() == want[f, :n].tobytes(), (cam, f)
                assert (out[f, n:].view(np.uint8) == 0x5A).all(), "records beyond the count were written"
                for name in ("size", "angle", "response", "octave"):
                    assert np.array_equal(out[f, :n][name], kp[f, :n][name])
            r.points_batch_device(d_in, d_n, RC.KP_STRIDE, 3, None, cam)          # in place
            assert r.status() == 0
            assert d_in.cpu().numpy().tobytes() == want.tobytes()
            assert r.points(kp[2], cam).tobytes() == want[2].tobytes()            # the host form
            assert np.isfinite(want["x"]).all() and np.isfinite(want["y"]).all()
        bad = np.array([RC.KP_STRIDE, RC.KP_STRIDE + 1, 1], np.int32)
        d_in, d_n = _dev(torch, work, kp), _dev(torch, work, bad)
        r.points_batch_device(d_in, d_n, RC.KP_STRIDE, 3, None, 1)
        assert r.status() == -1                                                    # ARIA_E_INVALID, once
        assert r.status() == 0
        assert d_in.cpu().numpy().tobytes() == RC.ref_points(1, kp, bad).tobytes()
    finally:
        r.close()


# ---- the read forms, the frame groups and the limits (rectify_cases.EDGE_CASES) ---------------------------------------------
@pytest.fixture(scope="module", params=RC.DEVICE_CASES)
def edge(request, aria, work):
    case = RC.EDGE_CASES[request.param]
    r = aria.HipRectifier(cameras=case.cam, new_K=case.new_K, src_size=case.src, dst_size=case.dst, fill=case.fill,
                          stream=work.cuda_stream)
    yield case, r
    r.close()


def _case_batch(torch, work, case, r, frames):
    """The batch form on the case's layouts -> (images, True when no padding byte changed)."""
    n = len(frames)
    d_src = _dev(torch, work, case.src_buffer(frames))
    d_dst = _full(torch, work, n * case.dst_stride, 0x5A)
    r.remap_batch_device(d_src, n, d_dst, 0, case.src_stride, case.src_pitch, case.dst_stride, case.dst_pitch)
    assert r.status() == 0
    return case.images(d_dst.cpu().numpy(), n)


def test_edge_case_map_equals_the_restatement(edge):
    """k3 != 0, quarter turns and a camera that looks away (Z <= 0), 8x8 and 2x2 sources, ix = iy = 2045 with bit 31 set."""
    case, r = edge
    got = r.map(0)
    print("%s: %d of %d words differ" % (case.name, int((got != case.map).sum()), got.size))
    assert got.tobytes() == case.map.tobytes()
    assert r.status() == 0


def test_edge_case_remap_equals_the_restatement(torch_cuda, work, edge):
    """Every frame of the case in one call (17 frames: blockIdx.z = 0, 1, 2 and a last group of one), then frame 8 and frame
    16 -- the first of the second group and the lone one of the third -- in calls of their own, the blocking host form on the
    last frame, and a call without frames."""
    case, r = edge
    img, pad_kept = _case_batch(torch_cuda, work, case, r, case.frames)
    print("%s: %d of %d pixels differ" % (case.name, int((img != case.want).sum()), case.want.size))
    assert img.tobytes() == case.want.tobytes()
    assert pad_kept, "padding was written"
    for f in sorted({8, 16} & set(range(case.n_frames))):
        one, pad_kept = _case_batch(torch_cuda, work, case, r, case.frames[f:f + 1])
        assert one.tobytes() == img[f:f + 1].tobytes() and pad_kept, f
    last = case.n_frames - 1
    assert r.remap(case.frames[last], 0).tobytes() == img[last].tobytes()
    d_src = _dev(torch_cuda, work, case.src_buffer(case.frames[:1]))
    d_dst = _full(torch_cuda, work, case.dst_stride, 0x5A)
    r.remap_batch_device(d_src, 0, d_dst, 0, case.src_stride, case.src_pitch, case.dst_stride, case.dst_pitch)
    assert r.status() == 0 and bool((d_dst == 0x5A).all()), "a call without frames wrote"


def test_edge_case_refuses_bad_layouts_before_a_launch(aria, torch_cuda, work, edge):
    """ARIA_E_INVALID, nothing enqueued and the destination untouched: a source or destination pitch below the width, a source
    pitch above 2^19, a stride that lets two frames overlap, a camera the handle does not have."""
    case, r = edge
    (sw, sh), (dw, dh) = case.src, case.dst
    d_src = _dev(torch_cuda, work, case.src_buffer(case.frames[:2] if case.n_frames > 1 else np.repeat(case.frames, 2, axis=0)))
    d_dst = _full(torch_cuda, work, 2 * case.dst_stride, 0x5A)
    good = dict(cam=0, src_stride=case.src_stride, src_pitch=case.src_pitch, dst_stride=case.dst_stride, dst_pitch=case.dst_pitch)
    bad = [dict(src_pitch=sw - 1), dict(src_pitch=(1 << 19) + 1), dict(dst_pitch=dw - 1),
           dict(src_stride=case.src_pitch * (sh - 1) + sw - 1), dict(dst_stride=case.dst_pitch * (dh - 1) + dw - 1),
           dict(cam=1), dict(cam=-1)]
    for kw in bad:
        with pytest.raises(aria.AriaError) as e:
            r.remap_batch_device(d_src, 2, d_dst, **dict(good, **kw))
        assert e.value.status == -1, kw
    with pytest.raises(aria.AriaError) as e:
        r.remap_batch_device(d_src, -1, d_dst, **good)
    assert e.value.status == -1
    with pytest.raises(aria.AriaError) as e:
        r.remap(case.frames[0], 1)
    assert e.value.status == -1
    assert r.status() == 0 and bool((d_dst == 0x5A).all()), "a refused call wrote"


def test_edge_points_equal_the_restatement(aria, torch_cuda, work):
    """NaN, infinite and huge keypoints and keypoints far outside the image, through an identity camera and two that look away
    (Ry(75), Ry(-100): Z <= 0 for about half the records): (-1, -1) wherever the restatement says so and nowhere else, out of
    place and in place, the host form; counts of (-1, 300) skip frame 0, leave its records as they are and report once."""
    torch = torch_cuda
    kp, counts = RC.edge_keypoints(), RC.POINT_COUNTS
    for name, cam in RC.point_cameras():
        want = RC.ref_edge_points_all()[name][0]
        r = aria.HipRectifier(cameras=cam, new_K=cam["K"], src_size=RC.SIZE, stream=work.cuda_stream)
        try:
            d_in, d_n = _dev(torch, work, kp), _dev(torch, work, counts)
            d_out = _full(torch, work, kp.nbytes, 0x5A)
            r.points_batch_device(d_in, d_n, RC.KP_STRIDE, 2, d_out)
            assert r.status() == 0
            out = d_out.cpu().numpy().view(kp.dtype).reshape(kp.shape)
            for f, n in enumerate(counts):
                gone = (want[f, :n]["x"] == -1) & (want[f, :n]["y"] == -1)
                print("%s frame %d: %d of %d at (-1, -1), %d records differ" % (name, f, int(gone.sum()), n, int((out[f, :n] != want[f, :n]).sum())))
                assert out[f, :n].tobytes() == want[f, :n].tobytes(), (name, f)
                assert (out[f, n:].view(np.uint8) == 0x5A).all(), "records beyond the count were written"
            r.points_batch_device(d_in, d_n, RC.KP_STRIDE, 2)                        # in place
            assert r.status() == 0
            assert d_in.cpu().numpy().tobytes() == want.tobytes(), name
            assert r.points(kp[1]).tobytes() == want[1].tobytes(), name               # the host form
            bad = np.array([-1, RC.KP_STRIDE], np.int32)
            d_in, d_n = _dev(torch, work, kp), _dev(torch, work, bad)
            r.points_batch_device(d_in, d_n, RC.KP_STRIDE, 2)
            assert r.status() == -1                                                   # ARIA_E_INVALID, once
            assert r.status() == 0
            got = d_in.cpu().numpy().view(kp.dtype).reshape(kp.shape)
            assert got[0].tobytes() == kp[0].tobytes(), "the skipped frame was written"
            assert got.tobytes() == RC.ref_edge_points(cam, kp, bad).tobytes(), name
        finally:
            r.close()


def test_chain_raw_pair_to_stereo_observations(aria, torch_cuda, work):
    """Shape (e): a raw synthetic pair at 320x240 -> device remap of both cameras -> extract_batch_device ->
    aria_stereo_match_batch_device, nothing leaving HBM in between. The rectified images equal the restatement's bytes and
    the stereo observations equal stereo_ref on those images."""
    from aria_slam_amd import rectify_ref as R
    from aria_slam_amd import stereo_ref as S
    from aria_slam_amd._lib import KP_DTYPE, MATCH_DTYPE, STEREO_OBS_DTYPE
    torch = torch_cuda
    W, H, NF, n = 320, 240, 500, 2
    cal = R.scaled_calibration(W, H, RC.EUROC)
    pairs = [R.raw_stereo_pair(seed, W, H, cal) for seed in (1, 2)]
    cl, cr, nk, baseline = R.rectified_cameras(cal)
    r = aria.HipRectifier.from_stereo_calibration(cal["K_l"], cal["D_l"], cal["T_BS_l"], cal["K_r"], cal["D_r"], cal["T_BS_r"],
                                                  (W, H), stream=work.cuda_stream)
    e = aria.OrbHipExtractor(max_features=NF, stream=work.cuda_stream, max_width=W, max_height=H, max_batch=n)
    st = aria.HipStereoMatcher(K=r.new_K, baseline=r.baseline, stream=work.cuda_stream)
    try:
        assert r.new_K == nk and r.baseline == baseline
        cap = e.kp_capacity()
        rect, side = [], []
        for cam, idx in ((0, 0), (1, 1)):
            d_raw = _dev(torch, work, np.stack([p[idx] for p in pairs]))
            d_img = _full(torch, work, n * W * H, 0x5A)
            r.remap_batch_device(d_raw, n, d_img, cam)
            k, d = _full(torch, work, n * cap * 24, 0), _full(torch, work, n * cap * 32, 0)
            c = _full(torch, work, 4 * n, 0).view(torch.int32)
            e.extract_batch_device(d_img, n, W, H, k, d, c, cap)
            e.check()
            rect.append(d_img)
            side.append((k, d, c))
        (d_kl, d_dl, d_nl), (d_kr, d_dr, d_nr) = side
        d_obs, d_m = _full(torch, work, n * cap * 32, 0x5A), _full(torch, work, n * cap * 12, 0x5A)
        d_nm = _full(torch, work, 4 * n, 0).view(torch.int32)
        st.match_batch_device(rect[0], rect[1], W * H, W, H, W, d_kl, d_dl, d_nl, d_kr, d_dr, d_nr, cap, n, d_obs, d_m, d_nm)
        assert st.status() == 0 and r.status() == 0
        imgs = [t.cpu().numpy().reshape(n, H, W) for t in rect]
        want_imgs = [np.stack([R.remap(p[idx], R.build_map(cam, nk, W, H, W, H)) for p in pairs])
                     for idx, cam in ((0, cl), (1, cr))]
        assert imgs[0].tobytes() == want_imgs[0].tobytes() and imgs[1].tobytes() == want_imgs[1].tobytes()
        nl, nr, nm = d_nl.cpu().numpy(), d_nr.cpu().numpy(), d_nm.cpu().numpy()
        kl, kr = (t.cpu().numpy().view(KP_DTYPE).reshape(n, cap) for t in (d_kl, d_kr))
        dl, dr = (t.cpu().numpy().reshape(n, cap, 32) for t in (d_dl, d_dr))
        obs = d_obs.cpu().numpy().view(STEREO_OBS_DTYPE).reshape(n, cap)
        m = d_m.cpu().numpy().view(MATCH_DTYPE).reshape(n, cap)
        for p in range(n):
            want_obs, want_m = S.stereo_match_ref(imgs[0][p], imgs[1][p], kl[p, :nl[p]], dl[p, :nl[p]], kr[p, :nr[p]],
                                                  dr[p, :nr[p]], K=r.new_K, baseline=r.baseline)
            assert obs[p, :nl[p]].tobytes() == want_obs.tobytes(), p
            assert nm[p] == len(want_m) and m[p, :nm[p]].tobytes() == want_m.tobytes(), p
            print("pair %d: %d of %d left keypoints matched" % (p, nm[p], nl[p]))
            assert nm[p] > 0.5 * nl[p] and nl[p] > 256                             # the chain works on a raw pair
    finally:
        st.close()
        e.close()
        r.close()
