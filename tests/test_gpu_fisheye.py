"""The fisheye model KB4 of the rectification stage on the MI355X (k_rect_build_map_kb4, k_rect_points_kb4 in
aria_slam_amd/csrc/rectify.hip, picked by aria_rect_config::model) against its definition, the NumPy restatement
aria_slam_amd/rectify_ref.py: every map word, every pixel and every keypoint field is BITWISE equal, through the C-ABI and
the Python binding. The cases are fisheye_cases.py's; the same cases run through the kernel text compiled for the host in
tests/test_fisheye_kernel_emulation.py: a case that fails here and passes there is a difference in the device's arithmetic
(rect_atan and rect_tan rest on the device's fp64 + - * / and sqrt being correctly rounded, as the radtan path does)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fisheye_cases as F   # noqa: E402
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


@pytest.fixture(scope="module", params=list(F.CASES))
def case_rect(request, aria, work):
    case = F.CASES[request.param]
    r = aria.HipRectifier(cameras=case.cam, new_K=case.new_K, src_size=case.src, dst_size=case.dst, fill=case.fill,
                          stream=work.cuda_stream)
    yield case, r
    r.close()


def test_map_equals_the_restatement(case_rect):
    """zoom10 (an invalid border), fold8 (invalid by the fold rule alone), yaw75 (Z <= 0), rig (a rectifying rotation), tele
    (a paraxial camera: rect_atan(r) / r at r below 4e-4)."""
    from aria_slam_amd import _lib
    case, r = case_rect
    assert r.model == "kb4" and r.config.model == _lib.RECT_MODEL_KB4 and r.camera(0) == case.cam
    got = r.map(0)
    print("%s: %d of %d words differ, %.3f invalid" % (case.name, int((got != case.map).sum()), got.size, (got == 0xFFFFFFFF).mean()))
    assert got.tobytes() == case.map.tobytes()
    assert r.status() == 0


def test_remap_equals_the_restatement(torch_cuda, work, case_rect):
    """Nine noise frames (groups of 8 and 1) in pitched, strided buffers; the destination prefilled 0x5A, its padding
    untouched; the lone frame of the second group in a call of its own; the blocking host form."""
    case, r = case_rect
    d_src = _dev(torch_cuda, work, case.src_buffer())
    d_dst = _full(torch_cuda, work, case.n_frames * case.dst_stride, 0x5A)
    r.remap_batch_device(d_src, case.n_frames, d_dst, 0, case.src_stride, case.src_pitch, case.dst_stride, case.dst_pitch)
    assert r.status() == 0
    img, pad_kept = case.images(d_dst.cpu().numpy())
    print("%s: %d of %d pixels differ" % (case.name, int((img != case.want).sum()), case.want.size))
    assert img.tobytes() == case.want.tobytes()
    assert pad_kept, "padding was written"
    d_one = _full(torch_cuda, work, case.dst_stride, 0x5A)
    r.remap_batch_device(_dev(torch_cuda, work, case.src_buffer(case.frames[8:9])), 1, d_one, 0, case.src_stride, case.src_pitch,
                         case.dst_stride, case.dst_pitch)
    assert r.status() == 0
    one, pad_kept = case.images(d_one.cpu().numpy(), 1)
    assert one.tobytes() == case.want[8:9].tobytes() and pad_kept
    assert r.remap(case.frames[0], 0).tobytes() == case.want[0].tobytes()


def test_rig_maps_of_both_cameras(aria, work):
    """from_stereo_calibration with model = "kb4": the geometry, both cameras' dicts and both maps."""
    from aria_slam_amd import rectify_ref as R
    g = F.RIG
    cl, cr, nk, baseline = R.rectified_cameras(g)
    r = aria.HipRectifier.from_stereo_calibration(g["K_l"], g["D_l"], g["T_BS_l"], g["K_r"], g["D_r"], g["T_BS_r"], F.SRC,
                                                  stream=work.cuda_stream, model="kb4")
    try:
        assert r.new_K == nk and r.baseline == baseline and r.camera(0) == cl and r.camera(1) == cr
        assert r.map(0).tobytes() == F.CASES["rig"].map.tobytes()
        assert r.map(1).tobytes() == R.build_map(cr, nk, F.SRC[0], F.SRC[1], F.SRC[0], F.SRC[1]).tobytes()
    finally:
        r.close()


@pytest.mark.parametrize("name,cam", F.point_cameras(), ids=[n for n, _ in F.point_cameras()])
def test_points_equal_the_restatement(aria, torch_cuda, work, name, cam):
    """Out of place and in place, records beyond the count untouched, every other field kept, the host form; a bad count
    skips its frame, leaves its records and is reported once."""
    torch = torch_cuda
    kp, counts = F.keypoints(), F.POINT_COUNTS
    want = F.ref_points_all()[name]
    r = aria.HipRectifier(cameras=cam, new_K=cam["K"], src_size=F.SRC, stream=work.cuda_stream)
    try:
        d_in, d_n = _dev(torch, work, kp), _dev(torch, work, counts)
        d_out = _full(torch, work, kp.nbytes, 0x5A)
        r.points_batch_device(d_in, d_n, F.KP_STRIDE, 2, d_out)
        assert r.status() == 0
        out = d_out.cpu().numpy().view(kp.dtype).reshape(kp.shape)
        for f, n in enumerate(counts):
            gone = (want[f, :n]["x"] == -1) & (want[f, :n]["y"] == -1)
            print("%s frame %d: %d of %d at (-1, -1), %d records differ" % (name, f, int(gone.sum()), n, int((out[f, :n] != want[f, :n]).sum())))
            assert out[f, :n].tobytes() == want[f, :n].tobytes(), (name, f)
            assert (out[f, n:].view(np.uint8) == 0x5A).all(), "records beyond the count were written"
            for field in ("size", "angle", "response", "octave"):
                assert np.array_equal(out[f, :n][field], kp[f, :n][field])
        r.points_batch_device(d_in, d_n, F.KP_STRIDE, 2)                            # in place
        assert r.status() == 0
        assert d_in.cpu().numpy().tobytes() == want.tobytes(), name
        assert r.points(kp[1]).tobytes() == want[1].tobytes(), name                   # the host form
        for bad in (np.array([-1, F.KP_STRIDE], np.int32), np.array([F.KP_STRIDE + 1, 1], np.int32)):
            d_in, d_n = _dev(torch, work, kp), _dev(torch, work, bad)
            r.points_batch_device(d_in, d_n, F.KP_STRIDE, 2)
            assert r.status() == -1                                                   # ARIA_E_INVALID, once
            assert r.status() == 0
            got = d_in.cpu().numpy().view(kp.dtype).reshape(kp.shape)
            assert got[0].tobytes() == kp[0].tobytes(), "the skipped frame was written"
            assert got.tobytes() == F.ref_points(cam, kp, bad).tobytes(), name
    finally:
        r.close()


def test_create_rejects_bad_models(aria):
    from aria_slam_amd import _lib
    L = aria.load_library()
    cfg = _lib.RectConfig()
    L.aria_rect_default_config(C.byref(cfg))
    cfg.src_width, cfg.src_height, cfg.dst_width, cfg.dst_height = 96, 64, 96, 64
    h = C.c_void_p()
    cfg.model = 2
    assert L.aria_rect_create(C.byref(cfg), C.byref(h)) == -1 and not h.value
    cfg.model = _lib.RECT_MODEL_KB4
    cfg.cam[0].dist[:] = list(F.D_A) + [0.01]
    assert L.aria_rect_create(C.byref(cfg), C.byref(h)) == -1 and not h.value
    cfg.cam[0].dist[4] = 0.0                                                           # and the same config without the fault
    assert L.aria_rect_create(C.byref(cfg), C.byref(h)) == 0 and h.value
    L.aria_rect_destroy(h)


def test_radtan_after_kb4_is_unchanged(aria, work):
    """A radtan handle created after a KB4 handle gives the existing 637x399 maps bitwise."""
    k = aria.HipRectifier(cameras=F.A, new_K=F.K_A, src_size=F.SRC, stream=work.cuda_stream)
    r = aria.HipRectifier.from_stereo_calibration(RC.K_L, RC.D_L, RC.T_BS_L, RC.K_R, RC.D_R, RC.T_BS_R, RC.SIZE, RC.SMALL,
                                                  RC.SMALL_NEW_K, stream=work.cuda_stream)
    try:
        assert k.model == "kb4" and r.model == "radtan" and "model" not in r.camera(0)
        for cam in range(2):
            assert r.map(cam).tobytes() == RC.ref_maps(True)[cam].tobytes(), cam
    finally:
        r.close()
        k.close()


def test_chain_raw_fisheye_pair_to_disparity(aria, torch_cuda, work):
    """Plumbing at 96x64: a raw fisheye pair by raw_from_rectified with the rig calibration -> device remap of both cameras
    -> HipDenseStereo. The rectified images equal the restatement's bytes, and the disparity map equals the one the same
    matcher computes from the restatement's rectified images, bit for bit."""
    from aria_slam_amd import rectify_ref as R
    from aria_slam_amd import stereo_ref as S
    torch = torch_cuda
    W, H = F.SRC
    left, right, _ = S.stereo_pair(5, W, H)
    raw = R.raw_from_rectified(left, right, F.RIG)
    cl, cr, nk, baseline = R.rectified_cameras(F.RIG)
    want = [R.remap(raw[k], R.build_map(cam, nk, W, H, W, H)) for k, cam in enumerate((cl, cr))]
    assert (want[0] != 0).mean() > 0.5 and (raw[0] != 110).mean() > 0.3                # the pair holds a scene
    r = aria.HipRectifier([cl, cr], nk, F.SRC, baseline=baseline, stream=work.cuda_stream)
    d = aria.HipDenseStereo(K=nk, baseline=baseline, max_size=(W, H))
    try:
        got = []
        for cam in range(2):
            d_img = _full(torch, work, W * H, 0x5A)
            r.remap_batch_device(_dev(torch, work, raw[cam]), 1, d_img, cam)
            assert r.status() == 0
            got.append(d_img.cpu().numpy().reshape(H, W))
            assert got[cam].tobytes() == want[cam].tobytes(), cam
        (disp, depth), (want_disp, want_depth) = d.compute(got[0], got[1]), d.compute(want[0], want[1])
        assert disp.tobytes() == want_disp.tobytes() and depth.tobytes() == want_depth.tobytes()
        assert disp.shape == (H, W)
    finally:
        d.close()
        r.close()
