"""Dense depth fusion on the MI355X (aria_tsdf_*, kernels in aria_slam_amd/csrc/tsdf_volume.hip) against its definition, the
NumPy restatement aria_slam_amd/tsdf_ref.py: every voxel byte and every point byte is BITWISE equal. The build rounds every
fp32 operation once and contracts nothing, so a difference is a bug, never a tolerance."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tsdf_cases as TC   # noqa: E402
from aria_slam_amd import tsdf_ref as R   # noqa: E402

ARIA_E_INVALID, ARIA_E_NO_DEVICE, ARIA_E_OUTPUT_TOO_SMALL = -1, -2, -5


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


def _handle(aria, work, cfg):
    return aria.HipTsdfVolume(dims=cfg.dims, voxel=cfg.voxel, origin=cfg.origin, trunc=cfg.trunc, min_depth=cfg.min_depth,
                              max_depth=cfg.max_depth, max_weight=cfg.max_weight, min_weight=cfg.min_weight, K=cfg.K,
                              stream=work.cuda_stream)


def _integrate(torch, work, h, depths, ext, images=None, mask=None):
    """One batch call over dense [n, H, W] inputs."""
    n, (H, W) = len(depths), depths[0].shape
    d_d = _dev(torch, work, np.ascontiguousarray(depths, np.float32))
    d_e = _dev(torch, work, np.ascontiguousarray(ext, np.float64))
    d_i = None if images is None else _dev(torch, work, np.ascontiguousarray(images, np.uint8))
    d_m = None if mask is None else _dev(torch, work, np.array(mask, np.uint8))
    h.integrate_batch_device(d_d, W, H, d_e, n, d_m, d_i)
    return h.status()


def _assert_equal(h, want_vol, want_pts, what):
    got = h.voxels()
    print("%s: %d of %d voxels differ, %d touched" % (what, int((got != want_vol).sum()), want_vol.size, int((want_vol["weight"] > 0).sum())))
    assert got.tobytes() == want_vol.tobytes(), what
    if want_pts is not None:
        pts = h.extract_points()
        print("%s: %d points, %d wanted" % (what, len(pts), len(want_pts)))
        assert pts.tobytes() == want_pts.tobytes(), what


@pytest.fixture(scope="module")
def scene_handle(aria, work):
    h = _handle(aria, work, TC.scene_config())
    yield h
    h.close()


def test_scene_equals_the_restatement(torch_cuda, work, scene_handle):
    """Shape (a): three poses of the plane and the sphere in one call, with images."""
    cfg, vol, pts = TC.ref_scene()
    d, im, e = TC.scene_frames()
    scene_handle.clear()
    assert _integrate(torch_cuda, work, scene_handle, d, e, im) == 0
    _assert_equal(scene_handle, vol, pts, "scene")
    assert len(pts) >= 400 and (vol["weight"] == 3).sum() > 1000
    # read_box: a box is the same records
    box = scene_handle.read_box(3, 5, 2, 17, 9, 11)
    assert box.tobytes() == np.ascontiguousarray(vol[2:13, 5:14, 3:20]).tobytes()
    # clear: every byte zero again, and no point
    scene_handle.clear()
    assert not scene_handle.voxels().view(np.uint8).any() and len(scene_handle.extract_points()) == 0


def test_small_volume_padded_layouts_and_bad_values(aria, torch_cuda, work):
    """Shape (b): 8 x 8 x 8 voxels under 5 x 3 depth maps; depth pitch 7 and image pitch 6 with padded strides (the depth padding
    holds a VALID depth, so reading it would show); depths of 0, negatives, NaN, +-Inf and one ulp outside [min_depth,
    max_depth]; the point buffer prefilled with a guard that survives beyond the written records."""
    torch = torch_cuda
    cfg, vol, pts = TC.ref_small()
    d, im, e = TC.small_frames()
    dl, il = (TC.SMALL_DEPTH_PITCH, TC.SMALL_DEPTH_STRIDE), (TC.SMALL_IMG_PITCH, TC.SMALL_IMG_STRIDE)
    d_d = _dev(torch, work, TC.padded(d, *dl, np.float32, np.float32(1.5)))
    d_i = _dev(torch, work, TC.padded(im, *il, np.uint8, TC.GUARD))
    d_e = _dev(torch, work, e)
    h = _handle(aria, work, cfg)
    try:
        h.integrate_batch_device(d_d, TC.SMALL_W, TC.SMALL_H, d_e, 3, None, d_i, depth_stride=dl[1], depth_pitch=dl[0],
                                 img_stride=il[1], img_pitch=il[0])
        assert h.status() == 0
        _assert_equal(h, vol, pts, "small")
        cap = len(pts) + 5
        d_p = _full(torch, work, 16 * cap, TC.GUARD)
        d_n = _full(torch, work, 8 * 3, TC.GUARD)
        h.extract_points_device(d_p, cap, d_n.data_ptr() + 8)
        assert h.status() == 0
        got = d_p.cpu().numpy().view(R.POINT_DTYPE)
        words = d_n.cpu().numpy().view(np.int64)
        assert got[:len(pts)].tobytes() == pts.tobytes() and (got[len(pts):].view(np.uint8) == TC.GUARD).all()
        assert words[1] == len(pts) and words[0] == words[2] == 0x5A5A5A5A5A5A5A5A
        assert (vol["weight"] > 0).sum() > 100 and len(pts) > 100
    finally:
        h.close()


def test_batch_split_host_form_and_frame_mask(aria, torch_cuda, work, scene_handle):
    """Shape (c): five frames in one call = five calls = groups of 2, 2, 1 = the host form; a mask of 1, 0, 1, 1, 0 = the three
    frames alone."""
    torch, h = torch_cuda, scene_handle
    cfg, vol, pts = TC.ref_five()
    d, im, e = TC.five_frames()
    for what, groups in (("one call", [slice(0, 5)]), ("five calls", [slice(k, k + 1) for k in range(5)]),
                         ("2, 2, 1", [slice(0, 2), slice(2, 4), slice(4, 5)])):
        h.clear()
        for g in groups:
            assert _integrate(torch, work, h, d[g], e[g], im[g]) == 0
        _assert_equal(h, vol, pts if what == "one call" else None, what)
    h.clear()
    for f in range(5):
        h.integrate(d[f], e[f], im[f])
    _assert_equal(h, vol, pts, "host form")
    keep = [0, 2, 3]
    want = TC.ref_integrated(cfg, d[keep], e[keep], im[keep])[0]
    h.clear()
    assert _integrate(torch, work, h, d, e, im, mask=[1, 0, 1, 1, 0]) == 0
    _assert_equal(h, want, None, "mask")
    h.clear()
    assert _integrate(torch, work, h, d[keep], e[keep], im[keep]) == 0
    _assert_equal(h, want, None, "three alone")
    assert want.tobytes() != vol.tobytes()


def test_seventy_frames_in_one_call(aria, torch_cuda, work):
    """More than 32 frames: three words of tile masks per tile, the last with 6 bits; every seventh camera looks away;
    max_weight = 20 is reached."""
    cfg, vol, pts = TC.ref_many()
    d, im, e = TC.many_frames()
    h = _handle(aria, work, cfg)
    try:
        assert _integrate(torch_cuda, work, h, d, e, im) == 0
        _assert_equal(h, vol, pts, "70 frames")
        assert vol["weight"].max() == 20
    finally:
        h.close()


def test_weight_cap_and_gray(aria, torch_cuda, work, scene_handle):
    """Shape (d): max_weight = 2 over five frames; gray with and without an image."""
    torch = torch_cuda
    cfg, vol, pts = TC.ref_five(max_weight=2)
    d, im, e = TC.five_frames()
    h = _handle(aria, work, cfg)
    try:
        assert _integrate(torch, work, h, d, e, im) == 0
        _assert_equal(h, vol, pts, "max_weight 2")
        assert vol["weight"].max() == 2 and (vol["weight"] == 2).sum() > 1000
    finally:
        h.close()
    want = TC.ref_integrated(TC.scene_config(), d, e)[0]
    scene_handle.clear()
    assert _integrate(torch, work, scene_handle, d, e) == 0
    _assert_equal(scene_handle, want, None, "no image")
    assert (want["gray"] == 0).all() and (TC.ref_five()[1]["gray"] != 0).any()
    # gray of an earlier call survives a call without an image; tsdf and weight go on
    want2 = TC.ref_five()[1].copy()
    R.integrate_batch(want2, TC.scene_config(), d[:2], e[:2])
    scene_handle.clear()
    assert _integrate(torch, work, scene_handle, d, e, im) == 0 and _integrate(torch, work, scene_handle, d[:2], e[:2]) == 0
    _assert_equal(scene_handle, want2, None, "image then none")


@pytest.mark.parametrize("name", sorted(TC.FRUSTUM_POSES))
def test_frustum_poses(aria, torch_cuda, work, name):
    """Shape (e): the camera inside the volume, the volume half behind the camera, entirely out of view (no byte changes), 0.5
    rad of yaw and pitch so that tiles straddle all four image borders, and a narrow view that leaves whole tiles beside the
    frustum. The kernel skips tiles outside the frustum, the restatement does not cull."""
    cfg, vol, pts = TC.ref_frustum(name)
    d, im, e = TC.frustum_frame(name)
    h = _handle(aria, work, cfg)
    try:
        assert _integrate(torch_cuda, work, h, d[None], e[None], im[None]) == 0
        _assert_equal(h, vol, pts, name)
        touched = int((vol["weight"] > 0).sum())
        assert touched == 0 if name == "outside" else touched > 100
    finally:
        h.close()


def test_extraction_edges(aria, torch_cuda, work, scene_handle):
    """Shape (f): an empty volume, a min_weight above every weight, a capacity below the total, a capacity of 0."""
    torch, h = torch_cuda, scene_handle
    cfg, vol, pts = TC.ref_scene()
    d, im, e = TC.scene_frames()
    h.clear()
    assert h.count_points() == 0 and len(h.extract_points()) == 0
    assert _integrate(torch, work, h, d, e, im) == 0
    total = len(pts)
    cap = total // 3
    got, n = h.extract_points(cap=cap)
    assert n == total and got.tobytes() == pts[:cap].tobytes()
    assert h.status() == 0                                           # the host form reported it already
    d_p = _full(torch, work, 16 * (cap + 2), TC.GUARD)
    d_n = _full(torch, work, 8, TC.GUARD)
    h.extract_points_device(d_p, cap, d_n)
    assert h.status() == ARIA_E_OUTPUT_TOO_SMALL and h.status() == 0             # deferred, reported once
    got = d_p.cpu().numpy().view(R.POINT_DTYPE)
    assert got[:cap].tobytes() == pts[:cap].tobytes() and (got[cap:].view(np.uint8) == TC.GUARD).all()
    assert d_n.cpu().numpy().view(np.int64)[0] == total
    h.extract_points_device(None, 0, d_n)                            # cap = 0: the count alone
    assert h.status() == ARIA_E_OUTPUT_TOO_SMALL and d_n.cpu().numpy().view(np.int64)[0] == total
    assert h.count_points() == total
    strict = _handle(aria, work, TC.scene_config(min_weight=4))      # three frames: no weight reaches 4
    try:
        assert _integrate(torch, work, strict, d, e, im) == 0
        assert strict.voxels().tobytes() == vol.tobytes() and strict.count_points() == 0
    finally:
        strict.close()


def test_chain_dense_depth_to_surface_points(aria, torch_cuda, work):
    """Shape (g): a synthetic rectified pair through aria_dense_compute_batch_device, its depth buffer handed straight to
    aria_tsdf_integrate_batch_device where it lies in HBM, then the extraction: equal to dense_ref followed by tsdf_ref."""
    import dense_cases as DC
    torch = torch_cuda
    Wd, Hd = DC.SCENE
    left, right, _ = DC.scene_pair(1, Wd, Hd)
    _, z = DC.ref(left, right)
    cfg = R.config(dims=(64, 32, 64), voxel=0.05, origin=(-2.4, -1.6, 0.8), trunc=0.15, K=DC.K, min_weight=1)
    e = TC.pose()
    want = R.new_volume(cfg)
    assert R.integrate(want, cfg, z, e, left)
    want_pts = R.extract(want, cfg)[0]
    dn = aria.HipDenseStereo(K=DC.K, baseline=DC.BASELINE, max_size=DC.SCENE, stream=work.cuda_stream)
    h = _handle(aria, work, cfg)
    try:
        d_l, d_r = _dev(torch, work, left), _dev(torch, work, right)
        d_disp = _full(torch, work, 2 * Wd * Hd, 0)
        d_z = _full(torch, work, 4 * Wd * Hd, 0)
        dn.compute_batch_device(d_l, d_r, Wd, Hd, 1, d_disp, d_z)
        h.integrate_batch_device(d_z, Wd, Hd, _dev(torch, work, e), 1, None, d_l)       # the same stream: ordered after the depth
        assert dn.status() == 0 and h.status() == 0
        _assert_equal(h, want, want_pts, "chain")
        assert (want["weight"] > 0).sum() > 1000 and len(want_pts) > 100
    finally:
        h.close()
        dn.close()


def test_non_finite_extrinsics_skip_their_frame(aria, torch_cuda, work, scene_handle):
    """Shape (h): one frame of three has a NaN in its extrinsics: that frame is skipped, ARIA_E_INVALID is reported once, the
    others are applied. The host form refuses such a frame and leaves the volume untouched."""
    torch, h = torch_cuda, scene_handle
    cfg = TC.scene_config()
    d, im, e = TC.scene_frames()
    bad = e.copy()
    bad[1, 5] = np.nan
    want = TC.ref_integrated(cfg, d[[0, 2]], e[[0, 2]], im[[0, 2]])[0]
    h.clear()
    assert _integrate(torch, work, h, d, bad, im) == ARIA_E_INVALID
    assert h.status() == 0
    _assert_equal(h, want, None, "non-finite")
    h.clear()
    assert _integrate(torch, work, h, d, bad, im, mask=[1, 0, 1]) == 0          # masked out: not an error
    _assert_equal(h, want, None, "non-finite, masked")
    with pytest.raises(aria.AriaError) as err:
        h.integrate(d[1], bad[1], im[1])
    assert err.value.status == ARIA_E_INVALID
    _assert_equal(h, want, None, "host form refused")


def test_lifecycle_and_refusals(aria, torch_cuda, work):
    """Shape (i): create refuses a bad struct size and a device that is not there; a borrowed stream is reported and survives
    close; a second close is a no-op; bad arguments are refused before anything is enqueued."""
    from aria_slam_amd import _lib
    torch = torch_cuda
    L = aria.load_library()
    cfg = _lib.TsdfConfig()
    L.aria_tsdf_default_config(C.byref(cfg))
    hh = C.c_void_p()
    cfg.struct_size += 4
    assert L.aria_tsdf_create(C.byref(cfg), C.byref(hh)) == ARIA_E_INVALID and not hh.value
    cfg.struct_size -= 4
    cfg.device = torch.cuda.device_count()
    assert L.aria_tsdf_create(C.byref(cfg), C.byref(hh)) == ARIA_E_NO_DEVICE and not hh.value
    assert ("device %d not present" % cfg.device) in L.aria_last_hip_error().decode()

    s = torch.cuda.Stream(device=torch.device("cuda", 0))
    h = aria.HipTsdfVolume(dims=(8, 8, 8), stream=s.cuda_stream)
    own = aria.HipTsdfVolume(dims=(8, 8, 8))
    try:
        assert h.stream == s.cuda_stream and own.stream and own.stream != s.cuda_stream
        for x in (h, own):
            assert x.status() == 0 and not x.voxels().view(np.uint8).any() and x.device_voxels()
            x.check()
        d_z = _full(torch, work, 4 * 8 * 8, 0)
        d_e = _dev(torch, work, TC.pose())
        call = lambda **kw: L.aria_tsdf_integrate_batch_device(   # noqa: E731
            h._h, kw.get("depth", d_z.data_ptr()), kw.get("stride", 64), kw.get("pitch", 8), kw.get("w", 8), kw.get("h", 8),
            kw.get("ext", d_e.data_ptr()), None, kw.get("img", None), 64, kw.get("img_pitch", 8), kw.get("n", 1))
        assert call() == 0 and call(n=0) == 0
        for kw in (dict(depth=None), dict(ext=None), dict(pitch=7), dict(w=0), dict(h=0), dict(w=16385, pitch=16385), dict(n=-1),
                   dict(n=65536), dict(n=2, stride=63), dict(img=d_z.data_ptr(), img_pitch=7)):
            assert call(**kw) == ARIA_E_INVALID, kw
        assert L.aria_tsdf_extract_points_device(h._h, None, 4, d_z.data_ptr()) == ARIA_E_INVALID
        assert L.aria_tsdf_extract_points_device(h._h, d_z.data_ptr(), -1, d_z.data_ptr()) == ARIA_E_INVALID
        assert L.aria_tsdf_extract_points_device(h._h, d_z.data_ptr(), 4, None) == ARIA_E_INVALID
        out = np.zeros(8, R.VOXEL_DTYPE)
        for box in ((-1, 0, 0, 1, 1, 1), (0, 0, 0, 9, 1, 1), (7, 0, 0, 2, 1, 1), (0, 0, 0, 1, 0, 1), (0, 0, 8, 1, 1, 1)):
            assert L.aria_tsdf_read_box(h._h, *box, out.ctypes.data) == ARIA_E_INVALID, box
        assert h.status() == 0
    finally:
        h.close()
        own.close()
    h.close()                                                        # a second close is a no-op
    with torch.cuda.stream(s):
        x = torch.arange(8, device="cuda:0") * 2
    s.synchronize()
    assert int(x.sum()) == 56


def test_export_ply_is_the_mappers_file_format(aria, torch_cuda, work, scene_handle, tmp_path):
    """export_ply writes HipMapper.export_ply's file: the same header text and vertex lines (mapper.ply_text on records with the
    same X and gray), one line per surface point of the restatement, in the canonical order."""
    from aria_slam_amd import mapper
    cfg, vol, pts = TC.ref_scene()
    d, im, e = TC.scene_frames()
    scene_handle.clear()
    assert _integrate(torch_cuda, work, scene_handle, d, e, im) == 0
    path = str(tmp_path / "surface.ply")
    scene_handle.export_ply(path)
    text = open(path).read()
    as_map = np.zeros(len(pts), mapper.MAP_POINT_DTYPE)              # what HipMapper would write for these positions and grays
    as_map["X"], as_map["gray"] = pts["X"], pts["gray"]
    assert text == mapper.ply_text(as_map)
    lines = text.splitlines(keepends=True)
    head = mapper.PLY_HEADER.format(n=len(pts))
    assert "".join(lines[:10]) == head and len(lines) == 10 + len(pts) and len(pts) >= 400
    for l, p in zip(lines[10:], pts):
        g = int(p["gray"])
        assert l == "%.6g %.6g %.6g %d %d %d\n" % (p["X"][0], p["X"][1], p["X"][2], g, g, g)
    assert len(set(int(g) for g in pts["gray"])) > 1                 # the images' gray reaches the file
    scene_handle.clear()
