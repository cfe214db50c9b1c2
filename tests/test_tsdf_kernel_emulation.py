"""The kernel source of aria_slam_amd/csrc/tsdf_volume.hip, compiled for the HOST and held bitwise to the restatement
(aria_slam_amd/tsdf_ref.py) on the shapes (a), (b) and (e) tests/test_gpu_tsdf.py runs on the device.

The text of the file between "namespace {" and the extraction section -- k_tsdf_prepare, k_tsdf_cull, k_tsdf_integrate and their device
functions -- is pasted between tests/cpp/tsdf_kernel_emu_head.inc (a shim: the lanes of a workgroup one after the other; the
two kernels have no barrier) and tsdf_kernel_emu_tail.inc (the parameters and the launch geometry) and compiled with the
clang++ that hipcc drives. What this checks without a GPU is the indexing, the tile geometry, the order of the fp32
operations as the host compiler takes them, the padded layouts and, above all, that the frustum test skips no voxel-frame the
restatement (which does not cull) touches; what it cannot check is the device's arithmetic, the extraction and the streams:
that is tests/test_gpu_tsdf.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tsdf_cases as TC   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/llvm/bin/clang++"


@pytest.fixture(scope="module")
def emu():
    src = open(os.path.join(ROOT, "aria_slam_amd", "csrc", "tsdf_volume.hip")).read()
    body = src[src.index("\nnamespace {"):src.index("\n// ---- extraction")]
    assert "k_tsdf_prepare" in body and "k_tsdf_integrate" in body and "k_tsdf_cull" in body
    assert "asm" not in body and "__shared__" not in body and "__syncthreads" not in body, "plain HIP C++, no LDS, no barrier"
    parts = [open(os.path.join(ROOT, "tests", "cpp", n)).read() for n in ("tsdf_kernel_emu_head.inc", "tsdf_kernel_emu_tail.inc")]
    out_dir = os.path.join(ROOT, "build", "tsdf_emu")
    os.makedirs(out_dir, exist_ok=True)
    cpp, so = os.path.join(out_dir, "tsdf_emu.cpp"), os.path.join(out_dir, "libtsdf_emu.so")
    with open(cpp, "w") as f:
        f.write(parts[0] + body + parts[1])
    assert os.path.exists(CLANG), "the clang++ of the ROCm installation (the one hipcc drives) is needed"
    subprocess.check_call([CLANG, "-std=c++17", "-O1", "-ffp-contract=off", "-fPIC", "-shared", "-w", "-o", so, cpp])
    L = C.CDLL(so)
    p, i, i64 = C.c_void_p, C.c_int, C.c_int64
    L.emu_integrate.argtypes = [p, p, p, p, p, i, p, i64, i, p, i64, i, i, i, p, p, p]
    L.emu_integrate.restype = None
    return L


def _run(L, cfg, depth, ext, size, images=None, mask=None, depth_layout=None, img_layout=None, cull=1, vol=None, group=0):
    """One call of the emulated pair of kernels over n frames. depth / images: [n, stride] buffers with their (pitch, stride),
    or [n, H, W] arrays. Returns (volume, error word)."""
    n = len(ext)
    W, H = size
    d = np.ascontiguousarray(depth, np.float32)
    dp, ds = depth_layout or (W, W * H)
    ip_, is_ = img_layout or (W, W * H)
    im = None if images is None else np.ascontiguousarray(images, np.uint8)
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    ip = np.array(list(cfg.dims) + [cfg.max_weight, W, H], np.int32)
    fp = np.array([cfg.voxel, *cfg.origin, cfg.trunc, cfg.min_depth, cfg.max_depth], np.float32)
    K = np.array(cfg.K, np.float64)
    e = np.ascontiguousarray(ext, np.float64)
    if vol is None:
        vol = np.zeros(cfg.dims[::-1], TC.R.VOXEL_DTYPE)
    frames = np.zeros(n * L.emu_frame_bytes(), np.uint8)
    err = np.zeros(1, np.int32)
    L.emu_integrate(ip.ctypes.data, fp.ctypes.data, K.ctypes.data, e.ctypes.data, m.ctypes.data if m is not None else None, n,
                    d.ctypes.data, ds, dp, im.ctypes.data if im is not None else None, is_, ip_, cull, group, vol.ctypes.data,
                    frames.ctypes.data, err.ctypes.data)
    return vol, int(err[0])


def test_integrate_kernel_source_is_bitwise_the_restatement_on_the_scene(emu):
    """Shape (a): three poses in one call, with images; the same with the frustum test off; and one call per frame."""
    cfg, want, _ = TC.ref_scene()
    d, im, e = TC.scene_frames()
    for cull in (1, 0):
        got, err = _run(emu, cfg, d, e, (TC.W, TC.H), im, cull=cull)
        assert err == 0 and got.tobytes() == want.tobytes(), (cull, int((got != want).sum()))
    vol = None
    for f in range(3):
        vol, err = _run(emu, cfg, d[f:f + 1], e[f:f + 1], (TC.W, TC.H), im[f:f + 1], vol=vol)
    assert vol.tobytes() == want.tobytes()
    assert (want["weight"] == 3).sum() > 1000 and (want["weight"] == 0).sum() > 1000


def test_integrate_kernel_source_layouts_and_bad_values(emu):
    """Shape (b): 8 x 8 x 8 voxels under 5 x 3 depth maps with padded pitches and strides, depths of every bad kind; a frame
    mask; a non-finite extrinsic raises the error bit and skips its frame only."""
    cfg, want, _ = TC.ref_small()
    d, im, e = TC.small_frames()
    dl, il = (TC.SMALL_DEPTH_PITCH, TC.SMALL_DEPTH_STRIDE), (TC.SMALL_IMG_PITCH, TC.SMALL_IMG_STRIDE)
    dbuf = TC.padded(d, *dl, np.float32, np.float32(1.5))            # a VALID depth in the padding: reading it would show
    ibuf = TC.padded(im, *il, np.uint8, TC.GUARD)
    got, err = _run(emu, cfg, dbuf, e, (TC.SMALL_W, TC.SMALL_H), ibuf, depth_layout=dl, img_layout=il)
    assert err == 0 and got.tobytes() == want.tobytes(), int((got != want).sum())
    only = TC.ref_integrated(cfg, d[[0, 2]], e[[0, 2]], im[[0, 2]])[0]
    got, err = _run(emu, cfg, dbuf, e, (TC.SMALL_W, TC.SMALL_H), ibuf, mask=[1, 0, 7], depth_layout=dl, img_layout=il)
    assert err == 0 and got.tobytes() == only.tobytes()
    bad = e.copy()
    bad[1, 3] = np.inf
    got, err = _run(emu, cfg, dbuf, bad, (TC.SMALL_W, TC.SMALL_H), ibuf, depth_layout=dl, img_layout=il)
    assert err == 1 and got.tobytes() == only.tobytes()
    got, err = _run(emu, cfg, dbuf, bad, (TC.SMALL_W, TC.SMALL_H), ibuf, mask=[1, 0, 1], depth_layout=dl, img_layout=il)
    assert err == 0 and got.tobytes() == only.tobytes()
    noimg = TC.ref_integrated(cfg, d, e)[0]
    got, err = _run(emu, cfg, dbuf, e, (TC.SMALL_W, TC.SMALL_H), depth_layout=dl)
    assert got.tobytes() == noimg.tobytes() and (got["gray"] == 0).all()


def test_integrate_kernel_source_seventy_frames_in_words_and_groups(emu):
    """70 frames: three words of tile masks in one launch, and the groups of 32 and 64 frames a call is cut into when its
    words do not fit the mask buffer. max_weight = 20 is reached."""
    cfg, want, _ = TC.ref_many()
    d, im, e = TC.many_frames()
    for group in (0, 32, 64):
        got, err = _run(emu, cfg, d, e, (TC.SMALL_W, TC.SMALL_H), im, group=group)
        assert err == 0 and got.tobytes() == want.tobytes(), (group, int((got != want).sum()))
    assert want["weight"].max() == 20 and (want["weight"] > 0).sum() > 300


@pytest.mark.parametrize("name", sorted(TC.FRUSTUM_POSES))
def test_integrate_kernel_source_frustum_poses(emu, name):
    """Shape (e): the camera inside the volume, the volume half behind the camera, entirely out of view, turned by 0.5 rad of
    yaw and pitch so that tiles straddle all four image borders, and a narrow view that leaves whole tiles beside the frustum.
    The restatement does not cull."""
    cfg, want, _ = TC.ref_frustum(name)
    d, im, e = TC.frustum_frame(name)
    got, err = _run(emu, cfg, d[None], e[None], TC.frustum_view(name)[0], im[None])
    assert err == 0 and got.tobytes() == want.tobytes(), int((got != want).sum())
    touched = int((want["weight"] > 0).sum())
    assert touched == 0 if name == "outside" else touched > 100
